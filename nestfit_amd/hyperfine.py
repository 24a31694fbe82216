"""Any species whose spectrum is a set of hyperfine lines under one excitation temperature, from a line table the caller
supplies: the reference's model-independent ``c_hf_predict`` (nestfit/models/hyperfine.pyx:52-118) with the parameters
of its N2H+ model per component -- voff, tex, ltau, sigm (diazenylium.pyx:138-154) -- on the kernels that ammonia and
N2H+ run on.  Only the line list changes: a rest frequency, velocity offsets and relative optical-depth weights.

No molecular data ship with this module: a `LineTable` is filled from a catalogue by its user (`LineTable.builtin` hands
out the shipped NH3 and N2H+ tables as templates).  The optical depth of line i of a component is 10**ltau * tau_wts[i]:
the weights are used as given, not normalised, and `ltau` is shared by the spectra of a pixel, so relative optical depths
between transitions are folded into the weights.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._model import (MODEL_AMMONIA, MODEL_DIAZENYLIUM, MODEL_HYPERFINE, EngineRunner, EngineSpectrumMixin,
                     check_options, spec_data_sizes_masked, par_names)
from .core import HyperfineSpectrum as _HyperfineBase

N_PARAMS = 4
MAX_LINES = 50            # NFA_MAX_HF_N
CKMS = 299792.458
_BUILTIN = {'ammonia': MODEL_AMMONIA, 'diazenylium': MODEL_DIAZENYLIUM}


class LineTable:
    """The lines of one transition: rest frequency `nu` (Hz), velocity offsets `voff` (km/s) and optical-depth weights
    `tau_wts` of its 1..50 lines, in any order.  Immutable; everything the engine would refuse raises ValueError here,
    before any device call."""
    __slots__ = ('_nu', '_voff', '_tau_wts', '_name')

    def __init__(self, nu, voff, tau_wts, name=None):
        try:
            nu = float(nu)
            voff = np.array(voff, dtype=np.float64)
            tau_wts = np.array(tau_wts, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f'a line table takes numbers: {e}') from None
        if voff.ndim != 1 or tau_wts.ndim != 1 or voff.shape != tau_wts.shape:
            raise ValueError(f'voff and tau_wts must be one-dimensional and of one length, not {voff.shape} and {tau_wts.shape}')
        if not 1 <= voff.size <= MAX_LINES:
            raise ValueError(f'a line table must have 1..{MAX_LINES} lines, not {voff.size}')
        if not (np.isfinite(nu) and nu > 0):
            raise ValueError(f'the rest frequency must be finite and positive, not {nu}')
        if not (np.all(np.isfinite(voff)) and np.all(np.abs(voff) < CKMS)):
            raise ValueError('every velocity offset must be finite and below the speed of light (km/s)')
        if not (np.all(np.isfinite(tau_wts)) and np.all(tau_wts >= 0)):
            raise ValueError('every line weight must be finite and not negative')
        if not np.any(tau_wts > 0):
            raise ValueError('the weights of a line table are all zero')
        voff.setflags(write=False)
        tau_wts.setflags(write=False)
        object.__setattr__(self, '_nu', nu)
        object.__setattr__(self, '_voff', voff)
        object.__setattr__(self, '_tau_wts', tau_wts)
        object.__setattr__(self, '_name', None if name is None else str(name))

    nu = property(lambda self: self._nu)
    voff = property(lambda self: self._voff)
    tau_wts = property(lambda self: self._tau_wts)
    name = property(lambda self: self._name)
    n = property(lambda self: int(self._voff.size))

    def __setattr__(self, key, value):
        raise AttributeError('a LineTable is immutable')

    def __delattr__(self, key):
        raise AttributeError('a LineTable is immutable')

    def __len__(self):
        return self.n

    def __eq__(self, other):
        """The same numbers in the same order (the name is a label)."""
        if not isinstance(other, LineTable):
            return NotImplemented
        return (self.nu == other.nu and np.array_equal(self.voff, other.voff)
                and np.array_equal(self.tau_wts, other.tau_wts))

    def __hash__(self):
        return hash((self.nu, self.voff.tobytes(), self.tau_wts.tobytes()))

    def __repr__(self):
        return f'LineTable(nu={self.nu!r}, {self.n} lines, name={self.name!r})'

    @classmethod
    def builtin(cls, model, trans_id):
        """A shipped table: model 'ammonia' (trans_id 1..9) or 'diazenylium' (1..3), through nfa_builtin_lines (no
        device needed).  A template for tables of one's own, and a table with known answers."""
        if model not in _BUILTIN:
            raise ValueError(f"shipped tables: {sorted(_BUILTIN)}, not {model!r}")
        nu, n = C.c_double(), C.c_int()
        voff, tau_wts = np.zeros(MAX_LINES), np.zeros(MAX_LINES)
        rc = _ffi.load().nfa_builtin_lines(_BUILTIN[model], int(trans_id), C.byref(nu), _ffi.dptr(voff),
                                           _ffi.dptr(tau_wts), C.byref(n))
        if rc != 0:
            raise ValueError(_ffi.load().nfa_last_error().decode())
        return cls(nu.value, voff[:n.value], tau_wts[:n.value], name=f'{model}:{int(trans_id)}')


class HyperfineSpectrum(EngineSpectrumMixin, _HyperfineBase):
    """A spectrum of the lines of `lines` (a `LineTable`).

    Parameters
    ----------
    xarr : array, Hz, ascending
    data : array, K
    noise : number, K; or one value per channel (inf masks a channel)
    lines : LineTable
    """
    MODEL = MODEL_HYPERFINE

    def __init__(self, xarr, data, noise, lines):
        if not isinstance(lines, LineTable):
            raise ValueError(f'`lines` must be a LineTable, not {type(lines).__name__}')
        _HyperfineBase.__init__(self, xarr, data, noise, rest_freq=lines.nu)
        self.lines = lines
        self._attach(-1, lines=lines)

    @property
    def tbg_arr(self):
        return self._ss.tbg()


def hf_predict(s, params):
    """Model spectrum of `s` for parameter-major `params` (voff, tex, ltau, sigm of every component; reference:
    hyperfine.pyx:52-118 as diazenylium.pyx:138-158 calls it); result in ``s.get_spec()`` / ``s.loglikelihood``."""
    s._predict(params, N_PARAMS)


class HyperfineRunner(EngineRunner):
    """Prior transform + model + log-likelihood of spectra with a `LineTable` each.  **options: the likelihood options of the
    spectra (`baseline_order`, `layered`, `calibration`, ...): see `_options`."""
    MODEL = MODEL_HYPERFINE
    N_MODEL = N_PARAMS

    def __init__(self, spectra, utrans, ncomp=1, **options):
        self.spectra = list(spectra)
        self._setup(self.spectra, utrans, ncomp, options=options)

    @classmethod
    def from_data(cls, spec_data, utrans, **kwargs):
        """spec_data: rows [xarr, data, noise, LineTable]."""
        check_options(kwargs, len(spec_data), *spec_data_sizes_masked(spec_data), model=cls.MODEL)     # before any device call
        spectra = np.array([HyperfineSpectrum(*args) for args in spec_data])
        return cls(spectra, utrans, **kwargs)

    def get_spectra(self):
        return np.array(self.spectra)

    def predict(self, params):
        params = self._check_params(params)
        if self._predict_through_set():
            return self._predict_layered(params)
        for s in self.spectra:
            hf_predict(s, params)


# Aliases and metadata at module scope, shaped like diazenylium.py's
N = N_PARAMS
IX_VCEN = 0
IX_SIGM = 3
NAME = 'hyperfine'
model_predict = hf_predict
ModelSpectrum = HyperfineSpectrum
ModelRunner = HyperfineRunner

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
