"""Non-LTE excitation from a grid of the caller's: every transition of a species has an excitation temperature and an
optical depth of its own, read from radiative-transfer tables (RADEX, LVG) over kinetic temperature, H2 density and column
density per line width -- so that lines which are fitted together BECAUSE their excitation differs (H2CO, HC3N, N2H+ 1-0
with 3-2, CS ladders) constrain the density instead of biasing a shared `tex`.  Parameters per component, parameter-major:

    voff (km/s), tkin (K), lnden = log10 n(H2)/cm^-3, lncol = log10 N/cm^-2, sigm (km/s)

An `ExcitationGrid` holds the three axes all spectra share: `tkin`, `lnden` and `lncd`, log10 of the column density per unit
line width, N / (cm^-2 (km/s)^-1), the width as FWHM -- the quantity such tables are computed over.  Every spectrum covers
one transition with any hyperfine structure inside it: a `GridLines`, a `LineTable` whose weights sum to 1 plus the two
tables `tex` (K) and `ltau` (log10 of the peak optical depth summed over the lines) on the grid.  For a component and a
spectrum s:

    x = (tkin, lnden, lncol - log10(sqrt(8 ln 2) sigm))
    per axis a_0 < ... < a_{n-1}:  k = #{ i in 1..n-2 : x >= a_i },  f = clamp((x - a_k) / (a_{k+1} - a_k), 0, 1)
                                   (one node: k = 0, f = 0 -- the axis has no effect)
    v(x) = trilinear over the eight corners, each step v0 + f (v1 - v0), lncd innermost, then lnden, then tkin
    tex_s = tex_s(x)       tau_main_s = 10 ** ltau_s(x)

and the spectrum follows as for the hyperfine model (the reference's c_hf_predict, nestfit/models/hyperfine.pyx:52-118)
with (voff, tex_s, tau_main_s, sigm).  OUTSIDE THE GRID THE EDGE VALUE HOLDS: nothing is extrapolated, so a prior that
leaves the grid sees a flat likelihood in that direction -- `ExcitationGrid.covers` says beforehand whether a prior box
stays inside.  A tkin, lnden or lncol that is not finite, or a sigm that is not an ordinary positive number, gives NaN.

No molecular data ship with this module and it reads no file format: the tables come from a code of the user's.
Out of scope: several transitions in one spectrum, several species on one grid, a filling factor, extrapolation.
"""
import numpy as np

from ._model import MODEL_GRID, EngineRunner, EngineSpectrumMixin, check_options, spec_data_sizes_masked, par_names
from ._options import refuse_unknown
from .core import HyperfineSpectrum as _HyperfineBase
from .hyperfine import LineTable

N_PARAMS = 5
MAX_NODES = 64            # NFA_GRID_MAXN
MAX_CELLS = 65536         # NFA_GRID_MAXCELLS
FWHM = 2.3548200450309493  # sqrt(8 ln 2): csrc/nfa_setup.h, NFA_GRID_FWHM
WEIGHT_SUM_TOL = 1e-6
_AXES = ('tkin', 'lnden', 'lncd')


def _cell(a, x):
    """(k, f) of the coordinates `x` on the axis `a`: the scan and the clamped fraction of the module's text.  A NaN
    coordinate keeps a NaN fraction."""
    n = a.size
    if n == 1:
        return np.zeros(x.shape, dtype=np.intp), np.zeros(x.shape)
    k = np.sum(x[..., None] >= a[1:n - 1], axis=-1)
    with np.errstate(invalid='ignore'):
        t = (x - a[k]) / (a[k + 1] - a[k])
        f = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    return k, f


class ExcitationGrid:
    """The axes of an excitation grid: `tkin` (K), `lnden` (log10 cm^-3) and `lncd` (log10 of cm^-2 per km/s of FWHM), each
    1..64 finite, strictly ascending nodes, at most 65536 together; a name.  Immutable and compared by value (the name is a
    label); everything the engine would refuse raises ValueError here."""
    __slots__ = ('_tkin', '_lnden', '_lncd', '_name')

    def __init__(self, tkin, lnden, lncd, name=None):
        axes = []
        for label, a in zip(_AXES, (tkin, lnden, lncd)):
            try:
                a = np.array(a, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f'an axis of an excitation grid takes numbers ({label}): {e}') from None
            if a.ndim != 1 or not 1 <= a.size <= MAX_NODES:
                raise ValueError(f'an axis of an excitation grid must be one-dimensional with 1..{MAX_NODES} nodes ({label}), '
                                 f'not of shape {a.shape}')
            if not (np.all(np.isfinite(a)) and np.all(np.diff(a) > 0)):
                raise ValueError(f'an axis of an excitation grid must be finite and strictly ascending ({label})')
            a.setflags(write=False)
            axes.append(a)
        if axes[0].size * axes[1].size * axes[2].size > MAX_CELLS:
            raise ValueError(f'an excitation grid must have at most {MAX_CELLS} nodes (nt * nn * nc), not '
                             f'{axes[0].size} * {axes[1].size} * {axes[2].size}')
        for key, value in zip(self.__slots__, (*axes, None if name is None else str(name))):
            object.__setattr__(self, key, value)

    tkin = property(lambda self: self._tkin)
    lnden = property(lambda self: self._lnden)
    lncd = property(lambda self: self._lncd)
    name = property(lambda self: self._name)
    shape = property(lambda self: (int(self._tkin.size), int(self._lnden.size), int(self._lncd.size)))

    def __setattr__(self, key, value):
        raise AttributeError('an ExcitationGrid is immutable')

    def __delattr__(self, key):
        raise AttributeError('an ExcitationGrid is immutable')

    def __eq__(self, other):
        if not isinstance(other, ExcitationGrid):
            return NotImplemented
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in _AXES)

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return hash(tuple(getattr(self, k).tobytes() for k in _AXES))

    def __repr__(self):
        return 'ExcitationGrid({} x {} x {} nodes, name={!r})'.format(*self.shape, self.name)

    def interpolate(self, table, tkin, lnden, lncd):
        """`table` [nt, nn, nc] at the coordinates (tkin, lnden, lncd), which broadcast: the module's trilinear rule with
        numpy in doubles, clamped at the edges."""
        table = np.asarray(table, dtype=np.float64)
        if table.shape != self.shape:
            raise ValueError(f'a table of this grid has the shape {self.shape}, not {table.shape}')
        xt, xn, xc = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (tkin, lnden, lncd)))
        (kt, ft), (kn, fn), (kc, fc) = _cell(self._tkin, xt), _cell(self._lnden, xn), _cell(self._lncd, xc)
        kt1, kn1, kc1 = (k + 1 if n > 1 else k for k, n in zip((kt, kn, kc), self.shape))
        with np.errstate(invalid='ignore'):
            def along_c(a, b):
                return table[a, b, kc] + fc * (table[a, b, kc1] - table[a, b, kc])
            v00, v01, v10, v11 = along_c(kt, kn), along_c(kt, kn1), along_c(kt1, kn), along_c(kt1, kn1)
            v0 = v00 + fn * (v01 - v00)
            v1 = v10 + fn * (v11 - v10)
            out = v0 + ft * (v1 - v0)
        return out if out.ndim else float(out)

    def covers(self, lower, upper):
        """Whether a prior box of the model's parameters stays inside the grid: `lower` and `upper` as `lsq.prior_box` gives
        them, parameter-major [5 ncomp] (voff, tkin, lnden, lncol, sigm of every component).  Every corner is asked, the
        sigm-dependent ones of lncd = lncol - log10(sqrt(8 ln 2) sigm) included; an axis of one node has no effect and covers
        everything.  Beyond the grid the model holds the edge value: the likelihood is flat there."""
        lower, upper = (np.asarray(v, dtype=np.float64).reshape(N_PARAMS, -1) for v in (lower, upper))
        if lower.shape != upper.shape or lower.shape[1] == 0:
            raise ValueError(f'a prior box is two arrays of {N_PARAMS} values per component')
        if not (np.all(lower[4] > 0) and np.all(np.isfinite(lower)) and np.all(np.isfinite(upper)) and np.all(upper >= lower)):
            return False
        boxes = ((self._tkin, lower[1], upper[1]), (self._lnden, lower[2], upper[2]),
                 (self._lncd, lower[3] - np.log10(FWHM * upper[4]), upper[3] - np.log10(FWHM * lower[4])))
        return bool(all(a.size == 1 or (np.all(lo >= a[0]) and np.all(hi <= a[-1])) for a, lo, hi in boxes))

    def transition(self, nu, tex, ltau, voff=None, tau_wts=None, name=None, normalise=False):
        """One transition on this grid as a `GridLines`: rest frequency `nu` (Hz), the tables `tex` (K) and `ltau` (log10 of
        the peak optical depth summed over the lines), [nt, nn, nc] each, and its hyperfine lines (none given: one line)."""
        return GridLines(self, nu, tex, ltau, (0.0,) if voff is None else voff, (1.0,) if tau_wts is None else tau_wts,
                         name=name, normalise=normalise)


class GridLines(LineTable):
    """The lines of one transition on an `ExcitationGrid`: a `LineTable` whose weights sum to 1 (within 1e-6; with
    `normalise=True` they are divided by their sum), plus the tables `tex` and `ltau` over the grid.  Every `tex` is finite
    and positive, every `ltau` finite.  Immutable and compared by value."""
    __slots__ = ('_grid', '_tex', '_ltau')

    def __init__(self, grid, nu, tex, ltau, voff=(0.0,), tau_wts=(1.0,), name=None, normalise=False):
        if not isinstance(grid, ExcitationGrid):
            raise ValueError(f'`grid` must be an ExcitationGrid, not {type(grid).__name__}')
        if normalise:
            LineTable.__init__(self, nu, voff, tau_wts, name=name)       # its checks first: a sum that can divide
            tau_wts = self.tau_wts / self.tau_wts.sum()
        LineTable.__init__(self, nu, voff, tau_wts, name=name)
        total = float(self.tau_wts.sum())
        if not abs(total - 1.0) <= WEIGHT_SUM_TOL:
            raise ValueError(f'the weights of a transition must sum to 1 within {WEIGHT_SUM_TOL:g} (normalise=True divides '
                             f'them by their sum), not {total!r}')
        tables = []
        for label, t in (('tex', tex), ('ltau', ltau)):
            try:
                t = np.array(t, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f'a table of an excitation grid takes numbers ({label}): {e}') from None
            if t.shape != grid.shape:
                raise ValueError(f'a table of this grid has the shape {grid.shape} ({label}), not {t.shape}')
            t.setflags(write=False)
            tables.append(t)
        if not (np.all(np.isfinite(tables[0])) and np.all(tables[0] > 0)):
            raise ValueError('every excitation temperature of a grid must be finite and positive: cut the grid where the '
                             'populations invert or the solver did not converge')
        if not np.all(np.isfinite(tables[1])):
            raise ValueError('every log10 optical depth of a grid must be finite: cut the grid where it is not')
        for key, value in zip(self.__slots__, (grid, *tables)):
            object.__setattr__(self, key, value)

    grid = property(lambda self: self._grid)
    tex = property(lambda self: self._tex)
    ltau = property(lambda self: self._ltau)

    def __setattr__(self, key, value):
        raise AttributeError('a GridLines is immutable')

    def __delattr__(self, key):
        raise AttributeError('a GridLines is immutable')

    def __eq__(self, other):
        """The same numbers in the same order on the same grid (the names are labels)."""
        if not isinstance(other, LineTable):
            return NotImplemented
        if not isinstance(other, GridLines):
            return False
        return (LineTable.__eq__(self, other) and self.grid == other.grid and np.array_equal(self.tex, other.tex)
                and np.array_equal(self.ltau, other.ltau))

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return hash((LineTable.__hash__(self), hash(self.grid), self.tex.tobytes(), self.ltau.tobytes()))

    def __repr__(self):
        return f'GridLines(nu={self.nu!r}, {self.n} lines on {self.grid!r}, name={self.name!r})'

    def excitation(self, tkin, lnden, lncol, sigm):
        """(tex, tau_main) of the transition for kinetic temperature `tkin` (K), `lnden` (log10 cm^-3), `lncol` (log10
        cm^-2) and `sigm` (km/s); numpy, broadcasting.  tau_main is NaN where tkin, lnden or lncol is not finite or sigm is
        not an ordinary positive number; tex is the module's rule in IEEE arithmetic whatever the arguments (an infinite
        coordinate clamps to the edge, a NaN one gives NaN unless its axis has one node)."""
        tkin, lnden, lncol, sigm = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (tkin, lnden, lncol, sigm)))
        with np.errstate(invalid='ignore', divide='ignore'):
            lncd = lncol - np.log10(FWHM * sigm)
            tex = np.asarray(self.grid.interpolate(self.tex, tkin, lnden, lncd))
            tau = np.power(10.0, np.asarray(self.grid.interpolate(self.ltau, tkin, lnden, lncd)))
        ordinary = np.isfinite(tkin) & np.isfinite(lnden) & np.isfinite(lncol) & (sigm > 0) & np.isfinite(sigm)
        tau = np.where(ordinary, tau, np.nan)
        return (tex, tau) if tex.ndim else (float(tex), float(tau))


def check_one_grid(lines):
    """The `ExcitationGrid` the `GridLines` of a runner share; ValueError if one is no GridLines or they name different
    grids."""
    lines = list(lines)
    if not lines or not all(isinstance(t, GridLines) for t in lines):
        raise ValueError('the excitation-grid model takes one GridLines (ExcitationGrid.transition) per spectrum')
    if any(t.grid != lines[0].grid for t in lines[1:]):
        raise ValueError('the spectra of a grid runner share one ExcitationGrid (the same axes): '
                         + ', '.join(sorted({repr(t.grid.name) for t in lines})))
    return lines[0].grid


class GridSpectrum(EngineSpectrumMixin, _HyperfineBase):
    """A spectrum of one transition, `lines` (a `GridLines`).

    Parameters
    ----------
    xarr : array, Hz, ascending
    data : array, K
    noise : number, K; or one value per channel (inf masks a channel)
    lines : GridLines
    """
    MODEL = MODEL_GRID

    def __init__(self, xarr, data, noise, lines):
        if not isinstance(lines, GridLines):
            raise ValueError(f'`lines` must be a GridLines, not {type(lines).__name__}')
        _HyperfineBase.__init__(self, xarr, data, noise, rest_freq=lines.nu)
        self.lines = lines
        self._attach(-1, lines=lines)

    @property
    def tbg_arr(self):
        return self._ss.tbg()


def grid_predict(s, params):
    """Model spectrum of `s` for parameter-major `params` (voff, tkin, lnden, lncol, sigm of every component); result in
    ``s.get_spec()`` / ``s.loglikelihood``."""
    s._predict(params, N_PARAMS)


class GridRunner(EngineRunner):
    """Prior transform + model + log-likelihood of spectra with a `GridLines` each, all on one `ExcitationGrid`.  **options:
    the likelihood options of the spectra -- `baseline_order`, `layered` and `noise_uncertainty`; a set of this model takes
    no calibration, correlation, response, templates, continuum or robust likelihood: see `_options`."""
    MODEL = MODEL_GRID
    N_MODEL = N_PARAMS

    def __init__(self, spectra, utrans, ncomp=1, **options):
        refuse_unknown(options, 'GridRunner.__init__')       # (a keyword it does not take: before it looks at the lines)
        self.spectra = list(spectra)
        self.grid = check_one_grid([s.lines for s in self.spectra])
        self._setup(self.spectra, utrans, ncomp, options=options)

    @classmethod
    def from_data(cls, spec_data, utrans, **kwargs):
        """spec_data: rows [xarr, data, noise, GridLines]."""
        check_options(kwargs, len(spec_data), *spec_data_sizes_masked(spec_data), model=cls.MODEL)     # before any device call
        spec_data = list(spec_data)
        check_one_grid([row[3] for row in spec_data])
        spectra = np.array([GridSpectrum(*args) for args in spec_data])
        return cls(spectra, utrans, **kwargs)

    def get_spectra(self):
        return np.array(self.spectra)

    def predict(self, params):
        params = self._check_params(params)
        if self._predict_through_set():
            return self._predict_layered(params)
        for s in self.spectra:
            grid_predict(s, params)


# Aliases and metadata at module scope, shaped like lte.py's
N = N_PARAMS
IX_VCEN = 0
IX_SIGM = 4
NAME = 'grid'
model_predict = grid_predict
ModelSpectrum = GridSpectrum
ModelRunner = GridRunner

PAR_NAMES = ['voff', 'tkin', 'lnden', 'lncol', 'sigm']
PAR_NAMES_SHORT = ['v', 'Tk', 'ln', 'lN', 's']

TEX_LABELS = [
    r'$v_\mathrm{lsr}$',
    r'$T_\mathrm{kin}$',
    r'$\log(n)$',
    r'$\log(N)$',
    r'$\sigma_\mathrm{v}$',
]

TEX_LABELS_WITH_UNITS = [
    r'$v_\mathrm{lsr} \ [\mathrm{km\, s^{-1}}]$',
    r'$T_\mathrm{kin} \ [\mathrm{K}]$',
    r'$\log(n) \ [\mathrm{cm^{-3}}]$',
    r'$\log(N) \ [\mathrm{cm^{-2}}]$',
    r'$\sigma_\mathrm{v} \ [\mathrm{km\, s^{-1}}]$',
]


def get_par_names(ncomp=None):
    return par_names(PAR_NAMES_SHORT, ncomp)
