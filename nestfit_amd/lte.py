"""One species in local thermodynamic equilibrium across several rotational transitions: column density, excitation
temperature and a partition function give every transition its own optical depth, so that cubes of, say, the 1-0 and
3-2 lines of one field are ONE fit per pixel with `N` and `T_ex` as parameters.  Parameters per component,
parameter-major: voff (km/s), tex (K), lncol = log10 of the total column density (cm^-2), sigm (km/s).

Every spectrum covers one transition, with any hyperfine structure inside it (an `LteLines`: a `LineTable` whose
weights sum to 1, plus the upper level and the Einstein coefficient); the spectra of a runner share one `Molecule`,
the partition function on a table of temperatures.  In cgs units, with T0 = h nu / k:

    ln Q(T)  linear in ln T between the bracketing entries of the table; outside it the end segment's line continues
    N_u      = 10**lncol * g_up * exp(-e_up / tex) / Q(tex)
    tau_main = N_u * c^2 a_ul / (8 pi nu^2) * expm1(T0 / tex) * CKMS / (sigm * nu * sqrt(2 pi))

`tau_main` is the transition's peak optical depth summed over its lines; line i gets tau_main * tau_wts[i], and the
spectrum follows as for the hyperfine model (the reference's c_hf_predict, nestfit/models/hyperfine.pyx:52-118).

A spectrum may also cover SEVERAL transitions of the species at once -- the K components of a symmetric top in one
window -- as an `LteBand` (`Molecule.band`): 1..8 `LteLines`, each with offsets from its own rest frequency, at most 50
lines together.  Line i of transition g then has

    hf_freq_i = (1 - voff_i / CKMS) * nu_g
    tau_i     = tau_main_g(tex, lncol, sigm) * tau_wts_i

and the spectrum follows from all the lines together, blended or not.  The parameters stay the four above.

Several SPECIES that share voff, tex and sigm along the line of sight -- a molecule and its isotopologue, whose ladder
lies inside the main one's window and fixes its optical depth; the A and E species of one molecule -- are one fit with a
column density per species: `LteMix(species)` describes the model of an ordered list of 1..4 `Molecule`s, an `LteBlend`
the transitions of any of them that one spectrum covers.  Parameters per component, parameter-major, 3 + K of them:

    voff, tex, lncol (species 0), sigm, lncol2 (species 1), ..., lncolK (species K - 1)

and a transition of species k has the tau_main above with lncol_k and Q_k(tex).  `LteBand`, `LteRunner` and
`check_one_molecule` stay what they were: one species.

All of the above assume that the gas fills the beam.  `LteMix(species, fill=True)` -- one species is the common case --
gives every component a BEAM FILLING FACTOR f as one more parameter, the last: `lnff` = log10 f, 4 + K per component,

    voff, tex, lncol, sigm, lncol2, ..., lncolK, lnff          Tb = sum_c 10^lnff_c T0 (y(T0 / tex_c) - tbg) (1 - e^-tau_c)

so that a thick line of a compact source reads f (J(tex) - J(Tbg)).  Nothing bounds f but the prior.  Where all lines are
optically thin the spectrum depends on f and the column densities only through f N: a thick line beside thin ones (a
main ladder and its isotopologue's) is what makes `lnff` identifiable.

No molecular data ship with this module: rest frequencies, level energies, Einstein coefficients and the partition
function come from a catalogue of the user's.
"""
import numpy as np

from ._model import MODEL_LTE, EngineRunner, EngineSpectrumMixin, check_options, spec_data_sizes_masked, par_names
from ._options import refuse_unknown
from .core import HyperfineSpectrum as _HyperfineBase
from .hyperfine import CKMS, MAX_LINES, LineTable

N_PARAMS = 4
MAX_TRANS = 8             # NFA_BAND_MAXT
MAX_SPECIES = 4           # NFA_LTE_MAXSP
MAX_Q = 64                # NFA_LTE_MAXQ
H_CGS = 6.62607015e-27    # csrc/nh3_data.h: NFA_H, NFA_KB, NFA_CCMS
KB_CGS = 1.380649e-16
CCMS = 29979245800.0
WEIGHT_SUM_TOL = 1e-6


class Molecule:
    """The partition function of a species: `q_val` at the 2..64 strictly ascending temperatures `q_temp` (K), and a
    name.  Immutable and compared by value; everything the engine would refuse raises ValueError here."""
    __slots__ = ('_name', '_q_temp', '_q_val', '_ln_t', '_ln_q', '_slope')

    def __init__(self, name, q_temp, q_val):
        try:
            q_temp = np.array(q_temp, dtype=np.float64)
            q_val = np.array(q_val, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f'a partition table takes numbers: {e}') from None
        if q_temp.ndim != 1 or q_val.ndim != 1 or q_temp.shape != q_val.shape:
            raise ValueError(f'q_temp and q_val must be one-dimensional and of one length, not {q_temp.shape} and {q_val.shape}')
        if not 2 <= q_temp.size <= MAX_Q:
            raise ValueError(f'a partition table must have 2..{MAX_Q} entries, not {q_temp.size}')
        if not (np.all(np.isfinite(q_temp)) and np.all(q_temp > 0) and np.all(np.diff(q_temp) > 0)):
            raise ValueError('the temperatures of a partition table must be finite, positive and strictly ascending')
        if not (np.all(np.isfinite(q_val)) and np.all(q_val > 0)):
            raise ValueError('every partition function value must be finite and positive')
        ln_t, ln_q = np.log(q_temp), np.log(q_val)
        if not np.all(np.diff(ln_t) > 0):
            raise ValueError('the temperatures of a partition table must be finite, positive and strictly ascending')
        slope = np.diff(ln_q) / np.diff(ln_t)
        for a in (q_temp, q_val, ln_t, ln_q, slope):
            a.setflags(write=False)
        for key, value in (('_name', str(name)), ('_q_temp', q_temp), ('_q_val', q_val), ('_ln_t', ln_t),
                           ('_ln_q', ln_q), ('_slope', slope)):
            object.__setattr__(self, key, value)

    name = property(lambda self: self._name)
    q_temp = property(lambda self: self._q_temp)
    q_val = property(lambda self: self._q_val)
    n = property(lambda self: int(self._q_temp.size))

    def __setattr__(self, key, value):
        raise AttributeError('a Molecule is immutable')

    def __delattr__(self, key):
        raise AttributeError('a Molecule is immutable')

    def __eq__(self, other):
        if not isinstance(other, Molecule):
            return NotImplemented
        return (self.name == other.name and np.array_equal(self.q_temp, other.q_temp)
                and np.array_equal(self.q_val, other.q_val))

    def __hash__(self):
        return hash((self.name, self.q_temp.tobytes(), self.q_val.tobytes()))

    def __repr__(self):
        return f'Molecule({self.name!r}, Q at {self.n} temperatures {self.q_temp[0]:g}..{self.q_temp[-1]:g} K)'

    def ln_partition(self, temp):
        """ln Q(T): linear in ln T inside the segment that brackets T, the end segments continued outside the table."""
        ln_temp = np.log(np.asarray(temp, dtype=np.float64))
        k = np.clip(np.searchsorted(self._ln_t, ln_temp, side='right') - 1, 0, self.n - 2)
        return self._ln_q[k] + self._slope[k] * (ln_temp - self._ln_t[k])

    def partition(self, temp):
        """Q(T), the log-log interpolation of the table."""
        return np.exp(self.ln_partition(temp))

    def transition(self, nu, e_up, g_up, a_ul, voff=(0.0,), tau_wts=(1.0,), name=None, normalise=False):
        """One transition of this species as an `LteLines`: rest frequency `nu` (Hz), upper-level energy `e_up` (K)
        and statistical weight `g_up`, Einstein coefficient `a_ul` (1/s), and its hyperfine lines."""
        return LteLines(self, nu, e_up, g_up, a_ul, voff, tau_wts, name=name, normalise=normalise)

    def band(self, transitions, name=None):
        """Several transitions of this species inside one spectrum, as an `LteBand`: 1..8 `LteLines` of this molecule."""
        return LteBand(self, transitions, name=name)


class LteLines(LineTable):
    """The lines of one rotational transition of a `Molecule`: a `LineTable` whose weights sum to 1 (within 1e-6; with
    `normalise=True` they are divided by their sum), plus `e_up` (K), `g_up` and `a_ul` (1/s).  Immutable."""
    __slots__ = ('_molecule', '_e_up', '_g_up', '_a_ul')

    def __init__(self, molecule, nu, e_up, g_up, a_ul, voff=(0.0,), tau_wts=(1.0,), name=None, normalise=False):
        if not isinstance(molecule, Molecule):
            raise ValueError(f'`molecule` must be a Molecule, not {type(molecule).__name__}')
        try:
            e_up, g_up, a_ul = float(e_up), float(g_up), float(a_ul)
        except (TypeError, ValueError) as e:
            raise ValueError(f'a transition takes numbers: {e}') from None
        if not (np.isfinite(e_up) and e_up >= 0):
            raise ValueError(f'the upper-level energy must be finite and not negative (K), not {e_up}')
        if not (np.isfinite(g_up) and g_up > 0):
            raise ValueError(f'the upper-level weight must be finite and positive, not {g_up}')
        if not (np.isfinite(a_ul) and a_ul > 0):
            raise ValueError(f'the Einstein coefficient must be finite and positive (1/s), not {a_ul}')
        if normalise:
            LineTable.__init__(self, nu, voff, tau_wts, name=name)       # its checks first: a sum that can divide
            tau_wts = self.tau_wts / self.tau_wts.sum()
        LineTable.__init__(self, nu, voff, tau_wts, name=name)
        total = float(self.tau_wts.sum())
        if not abs(total - 1.0) <= WEIGHT_SUM_TOL:
            raise ValueError(f'the weights of a transition must sum to 1 within {WEIGHT_SUM_TOL:g} (normalise=True divides '
                             f'them by their sum), not {total!r}')
        for key, value in (('_molecule', molecule), ('_e_up', e_up), ('_g_up', g_up), ('_a_ul', a_ul)):
            object.__setattr__(self, key, value)

    molecule = property(lambda self: self._molecule)
    e_up = property(lambda self: self._e_up)
    g_up = property(lambda self: self._g_up)
    a_ul = property(lambda self: self._a_ul)

    def __setattr__(self, key, value):
        raise AttributeError('an LteLines is immutable')

    def __delattr__(self, key):
        raise AttributeError('an LteLines is immutable')

    def __eq__(self, other):
        """The same numbers in the same order and the same molecule (the transition's name is a label)."""
        if not isinstance(other, LineTable):
            return NotImplemented
        if not isinstance(other, LteLines):
            return False
        return (LineTable.__eq__(self, other) and self.e_up == other.e_up and self.g_up == other.g_up
                and self.a_ul == other.a_ul and self.molecule == other.molecule)

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return hash((LineTable.__hash__(self), self.e_up, self.g_up, self.a_ul, hash(self.molecule)))

    def __repr__(self):
        return (f'LteLines({self.molecule.name!r}, nu={self.nu!r}, e_up={self.e_up!r}, g_up={self.g_up!r}, '
                f'a_ul={self.a_ul!r}, {self.n} lines, name={self.name!r})')

    def tau_main(self, tex, lncol, sigm):
        """The transition's peak optical depth summed over its lines, for `tex` (K), `lncol` (log10 cm^-2) and `sigm`
        (km/s); numpy, broadcasting."""
        tex, lncol, sigm = (np.asarray(a, dtype=np.float64) for a in (tex, lncol, sigm))
        nu = self.nu
        t0 = H_CGS * nu / KB_CGS
        pop_upper = 10.0 ** lncol * self.g_up * np.exp(-self.e_up / tex) / self.molecule.partition(tex)
        fracterm = CCMS * CCMS * self.a_ul / (8 * np.pi * (nu * nu))
        widthterm = CKMS / (sigm * nu * np.sqrt(2 * np.pi))
        return pop_upper * fracterm * np.expm1(t0 / tex) * widthterm


class LteBand:
    """The transitions of one `Molecule` that one spectrum covers: a sequence of 1..8 `LteLines` in the caller's order,
    at most 50 lines together, no transition twice.  Immutable, compared by value (the transitions in their order; the
    name is a label) and hashable; everything the engine would refuse raises ValueError here.  The order of the
    transitions does not change the model."""
    __slots__ = ('_molecule', '_transitions', '_name')

    def __init__(self, molecule, transitions, name=None):
        if not isinstance(molecule, Molecule):
            raise ValueError(f'`molecule` must be a Molecule, not {type(molecule).__name__}')
        try:
            transitions = tuple(transitions)
        except TypeError:
            raise ValueError('a band takes a sequence of LteLines') from None
        if not all(isinstance(t, LteLines) for t in transitions):
            raise ValueError('a band takes LteLines (Molecule.transition), one per transition')
        if not 1 <= len(transitions) <= MAX_TRANS:
            raise ValueError(f'a band must have 1..{MAX_TRANS} transitions, not {len(transitions)}')
        if any(t.molecule != molecule for t in transitions):
            raise ValueError('the transitions of a band are of one Molecule: '
                             + ', '.join(sorted({t.molecule.name for t in transitions} | {molecule.name})))
        n_lines = sum(t.n for t in transitions)
        if n_lines > MAX_LINES:
            raise ValueError(f'the transitions of a band must have at most {MAX_LINES} lines together, not {n_lines}')
        keys = [(t.nu, t.e_up, t.g_up, t.a_ul) for t in transitions]
        if len(set(keys)) != len(keys):
            raise ValueError('a band lists the same transition (nu, e_up, g_up, a_ul) twice')
        for key, value in (('_molecule', molecule), ('_transitions', transitions), ('_name', None if name is None else str(name))):
            object.__setattr__(self, key, value)

    molecule = property(lambda self: self._molecule)
    transitions = property(lambda self: self._transitions)
    name = property(lambda self: self._name)
    n_trans = property(lambda self: len(self._transitions))
    n_lines = property(lambda self: sum(t.n for t in self._transitions))
    n = n_lines                                                      # as a LineTable counts: the lines of the spectrum
    nu = property(lambda self: self._transitions[0].nu)             # the first transition's: axes and labels

    def __setattr__(self, key, value):
        raise AttributeError('an LteBand is immutable')

    def __delattr__(self, key):
        raise AttributeError('an LteBand is immutable')

    def __len__(self):
        return len(self._transitions)

    def __getitem__(self, k):
        return self._transitions[k]

    def __iter__(self):
        return iter(self._transitions)

    def __eq__(self, other):
        if not isinstance(other, LteBand):
            return NotImplemented
        return self._transitions == other._transitions

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return hash(('band',) + self._transitions)

    def __repr__(self):
        return (f'LteBand({self.molecule.name!r}, {self.n_trans} transitions at '
                f'{", ".join(format(t.nu, "g") for t in self._transitions)} Hz, {self.n_lines} lines, name={self.name!r})')

    def tau_main(self, tex, lncol, sigm):
        """The peak optical depth of every transition, in the band's order: numpy, one value per transition along the
        first axis, the arguments broadcasting behind it."""
        return np.stack([t.tau_main(tex, lncol, sigm) for t in self._transitions])


class LteBlend:
    """The transitions that one spectrum covers, of ANY `Molecule`s: a sequence of 1..8 `LteLines` in the caller's
    order, at most 50 lines together, no transition of a molecule twice.  For an `LteMix`; shaped like an `LteBand`:
    immutable, compared by value (the transitions in their order; the name is a label) and hashable; everything the
    engine would refuse raises ValueError here.  The order of the transitions does not change the model."""
    __slots__ = ('_transitions', '_name')

    def __init__(self, transitions, name=None):
        try:
            transitions = tuple(transitions)
        except TypeError:
            raise ValueError('a blend takes a sequence of LteLines') from None
        if not all(isinstance(t, LteLines) for t in transitions):
            raise ValueError('a blend takes LteLines (Molecule.transition), one per transition')
        if not 1 <= len(transitions) <= MAX_TRANS:
            raise ValueError(f'a blend must have 1..{MAX_TRANS} transitions, not {len(transitions)}')
        n_lines = sum(t.n for t in transitions)
        if n_lines > MAX_LINES:
            raise ValueError(f'the transitions of a blend must have at most {MAX_LINES} lines together, not {n_lines}')
        keys = [(t.molecule, t.nu, t.e_up, t.g_up, t.a_ul) for t in transitions]
        if len(set(keys)) != len(keys):
            raise ValueError('a blend lists the same transition (nu, e_up, g_up, a_ul) of a molecule twice')
        for key, value in (('_transitions', transitions), ('_name', None if name is None else str(name))):
            object.__setattr__(self, key, value)

    transitions = property(lambda self: self._transitions)
    name = property(lambda self: self._name)
    n_trans = property(lambda self: len(self._transitions))
    n_lines = property(lambda self: sum(t.n for t in self._transitions))
    n = n_lines                                                      # as a LineTable counts: the lines of the spectrum
    nu = property(lambda self: self._transitions[0].nu)             # the first transition's: axes and labels

    @property
    def molecules(self):
        """The distinct molecules of the transitions, in the order of their first appearance."""
        out = []
        for t in self._transitions:
            if t.molecule not in out:
                out.append(t.molecule)
        return tuple(out)

    def __setattr__(self, key, value):
        raise AttributeError('an LteBlend is immutable')

    def __delattr__(self, key):
        raise AttributeError('an LteBlend is immutable')

    def __len__(self):
        return len(self._transitions)

    def __getitem__(self, k):
        return self._transitions[k]

    def __iter__(self):
        return iter(self._transitions)

    def __eq__(self, other):
        if not isinstance(other, LteBlend):
            return NotImplemented
        return self._transitions == other._transitions

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return hash(('blend',) + self._transitions)

    def __repr__(self):
        return (f'LteBlend({", ".join(repr(m.name) for m in self.molecules)}: {self.n_trans} transitions at '
                f'{", ".join(format(t.nu, "g") for t in self._transitions)} Hz, {self.n_lines} lines, name={self.name!r})')


def transitions_of(lines):
    """The `LteLines` of a spectrum's `lines`: those of an `LteBand` or an `LteBlend`, or the one `LteLines` itself."""
    return lines.transitions if isinstance(lines, (LteBand, LteBlend)) else (lines,)


def check_one_molecule(lines):
    """The `Molecule` the `LteLines` and `LteBand`s of a runner share; ValueError if one is neither or they name
    different ones."""
    lines = list(lines)
    if not lines or not all(isinstance(t, (LteLines, LteBand)) for t in lines):
        raise ValueError('the LTE model takes one LteLines (Molecule.transition) or LteBand (Molecule.band) per spectrum')
    if any(t.molecule != lines[0].molecule for t in lines[1:]):
        raise ValueError('the spectra of an LTE runner share one Molecule (one species, one partition function): '
                         + ', '.join(sorted({t.molecule.name for t in lines})))
    return lines[0].molecule


class LteSpectrum(EngineSpectrumMixin, _HyperfineBase):
    """A spectrum of one transition, `lines` (an `LteLines`), or of several at once (an `LteBand`).

    Parameters
    ----------
    xarr : array, Hz, ascending
    data : array, K
    noise : number, K; or one value per channel (inf masks a channel)
    lines : LteLines or LteBand
    """
    MODEL = MODEL_LTE

    def __init__(self, xarr, data, noise, lines):
        if not isinstance(lines, (LteLines, LteBand)):
            raise ValueError(f'`lines` must be an LteLines or an LteBand, not {type(lines).__name__}')
        _HyperfineBase.__init__(self, xarr, data, noise, rest_freq=lines.nu)
        self.lines = lines
        self._attach(-1, lines=lines)

    @property
    def tbg_arr(self):
        return self._ss.tbg()


def lte_predict(s, params):
    """Model spectrum of `s` for parameter-major `params` (voff, tex, lncol, sigm of every component); result in
    ``s.get_spec()`` / ``s.loglikelihood``."""
    s._predict(params, N_PARAMS)


class LteRunner(EngineRunner):
    """Prior transform + model + log-likelihood of spectra with an `LteLines` or an `LteBand` each, all of one `Molecule`.
    **options: the likelihood options of the spectra (`baseline_order`, `layered`, `calibration`, ...): see `_options`."""
    MODEL = MODEL_LTE
    N_MODEL = N_PARAMS

    def __init__(self, spectra, utrans, ncomp=1, **options):
        refuse_unknown(options, 'LteRunner.__init__')        # (a keyword it does not take: before it looks at the lines)
        self.spectra = list(spectra)
        self.molecule = check_one_molecule([s.lines for s in self.spectra])
        self._setup(self.spectra, utrans, ncomp, options=options)

    @classmethod
    def from_data(cls, spec_data, utrans, **kwargs):
        """spec_data: rows [xarr, data, noise, LteLines or LteBand]."""
        check_options(kwargs, len(spec_data), *spec_data_sizes_masked(spec_data), model=cls.MODEL)     # before any device call
        spec_data = list(spec_data)
        check_one_molecule([row[3] for row in spec_data])
        spectra = np.array([LteSpectrum(*args) for args in spec_data])
        return cls(spectra, utrans, **kwargs)

    def get_spectra(self):
        return np.array(self.spectra)

    def predict(self, params):
        params = self._check_params(params)
        if self._predict_through_set():
            return self._predict_layered(params)
        for s in self.spectra:
            lte_predict(s, params)


# Aliases and metadata at module scope, shaped like hyperfine.py's
N = N_PARAMS
IX_VCEN = 0
IX_SIGM = 3
NAME = 'lte'
model_predict = lte_predict
ModelSpectrum = LteSpectrum
ModelRunner = LteRunner

PAR_NAMES = ['voff', 'tex', 'lncol', 'sigm']
PAR_NAMES_SHORT = ['v', 'Tx', 'lN', 's']

TEX_LABELS = [
    r'$v_\mathrm{lsr}$',
    r'$T_\mathrm{ex}$',
    r'$\log(N)$',
    r'$\sigma_\mathrm{v}$',
]

TEX_LABELS_WITH_UNITS = [
    r'$v_\mathrm{lsr} \ [\mathrm{km\, s^{-1}}]$',
    r'$T_\mathrm{ex} \ [\mathrm{K}]$',
    r'$\log(N) \ [\mathrm{cm^{-2}}]$',
    r'$\sigma_\mathrm{v} \ [\mathrm{km\, s^{-1}}]$',
]


def get_par_names(ncomp=None):
    return par_names(PAR_NAMES_SHORT, ncomp)


# ---------------------------------------------------------------------------- several species: one column density each
def check_species(species):
    """The ordered tuple of 1..4 distinct `Molecule`s of an `LteMix`; ValueError otherwise."""
    try:
        species = tuple(species)
    except TypeError:
        raise ValueError('the species of an LTE mix are a sequence of Molecules') from None
    if not all(isinstance(m, Molecule) for m in species):
        raise ValueError('the species of an LTE mix are Molecules')
    if not 1 <= len(species) <= MAX_SPECIES:
        raise ValueError(f'an LTE mix has 1..{MAX_SPECIES} species, not {len(species)}')
    if len(set(species)) != len(species):
        raise ValueError('an LTE mix lists a Molecule twice: ' + ', '.join(m.name for m in species))
    return species


def check_mix_lines(species, lines, all_species=True):
    """The `lines` of the spectra of a mix of `species` (an `LteLines`, `LteBand` or `LteBlend` each) as a list; ValueError
    if one is none of these, a transition is of a molecule that is no species of the mix, or (all_species) a species has
    no transition in any spectrum, which would leave its column density unconstrained."""
    species = check_species(species)
    lines = list(lines)
    if not lines or not all(isinstance(t, (LteLines, LteBand, LteBlend)) for t in lines):
        raise ValueError('an LTE mix takes one LteLines (Molecule.transition), LteBand or LteBlend per spectrum')
    seen = set()
    for k, table in enumerate(lines):
        for t in transitions_of(table):
            if t.molecule not in species:
                raise ValueError(f'spectrum {k} has a transition of {t.molecule.name!r}, which is no species of the mix ('
                                 + ', '.join(m.name for m in species) + ')')
            seen.add(species.index(t.molecule))
    if all_species and len(seen) != len(species):
        missing = ', '.join(m.name for k, m in enumerate(species) if k not in seen)
        raise ValueError(f'a species of the mix has no transition in any spectrum (its column density would be unconstrained): {missing}')
    return lines


def lines_species(lines):
    """The distinct molecules of the spectra's `lines`, in the order of their first appearance."""
    out = []
    for table in lines:
        for t in transitions_of(table):
            if t.molecule not in out:
                out.append(t.molecule)
    return tuple(out)


class _MixSpectrum(EngineSpectrumMixin, _HyperfineBase):
    """A spectrum of an `LteMix` (its `Spectrum`): `lines` an `LteLines`, an `LteBand` or an `LteBlend` of the mix's species.
    Its own model values (`LteMix.predict`) come from a set of this spectrum alone, with the species that have a transition
    in it."""
    MODEL = MODEL_LTE
    MIX = None

    def __init__(self, xarr, data, noise, lines):
        check_mix_lines(self.MIX.species, [lines], all_species=False)
        _HyperfineBase.__init__(self, xarr, data, noise, rest_freq=lines.nu)
        self.lines = lines
        present = [k for k, m in enumerate(self.MIX.species) if m in lines_species([lines])]
        # the rows of a component's parameters this spectrum's own set takes, in its order
        self._rows = [0, 1, self.MIX.lncol_row(present[0]), 3] + [self.MIX.lncol_row(k) for k in present[1:]]
        if self.MIX.fill:                                             # the filling factor: the last row, here as there
            self._rows.append(self.MIX.N - 1)
        self._attach(-1, lines=lines, species=[self.MIX.species[k] for k in present], fill=self.MIX.fill)

    @property
    def tbg_arr(self):
        return self._ss.tbg()


class _MixRunner(EngineRunner):
    """Prior transform + model + log-likelihood of the spectra of an `LteMix` (its `Runner`).  **options: the likelihood
    options of the spectra (`baseline_order`, `layered`, `calibration`, ...): see `_options`."""
    MODEL = MODEL_LTE
    MIX = None

    def __init__(self, spectra, utrans, ncomp=1, **options):
        refuse_unknown(options, '_MixRunner.__init__')
        self.spectra = list(spectra)
        check_mix_lines(self.MIX.species, [s.lines for s in self.spectra])
        self.species = self.MIX.species
        self._setup(self.spectra, utrans, ncomp, options=options)

    @classmethod
    def from_data(cls, spec_data, utrans, **kwargs):
        """spec_data: rows [xarr, data, noise, LteLines | LteBand | LteBlend]."""
        check_options(kwargs, len(spec_data), *spec_data_sizes_masked(spec_data), model=cls.MODEL)     # before any device call
        spec_data = list(spec_data)
        check_mix_lines(cls.MIX.species, [row[3] for row in spec_data])
        spectra = np.array([cls.MIX.Spectrum(*args) for args in spec_data])
        return cls(spectra, utrans, **kwargs)

    def get_spectra(self):
        return np.array(self.spectra)

    def predict(self, params):
        params = self._check_params(params)
        if self._predict_through_set():
            return self._predict_layered(params)
        for s in self.spectra:
            self.MIX.predict(s, params)


class LteMix:
    """The model of K = 1..4 species in LTE that share voff, tex and sigm, each with a column density of its own: an ordered
    list of distinct `Molecule`s.  Immutable, compared by the species.  What a model module offers, bound to the species:
    `N = 3 + K`, `NAME`, `IX_VCEN`, `IX_SIGM`, the parameter names and labels, `Runner`, `Spectrum`, `predict`.
    fill=True: with a beam filling factor per component as the last parameter, `lnff` = log10 f (`N = 4 + K`; `.fill`);
    a filled and an unfilled mix of the same species are different models."""
    NAME = 'lte_mix'
    IX_VCEN = 0
    IX_SIGM = 3

    def __init__(self, species, fill=False):
        species = check_species(species)
        if not isinstance(fill, (bool, np.bool_)):
            raise ValueError('`fill` is True or False: whether a component has a beam filling factor')
        fill = bool(fill)
        K = len(species)
        N = 3 + K + (1 if fill else 0)
        more = range(2, K + 1)
        attrs = {
            'species': species, 'N': N, 'fill': fill,
            'PAR_NAMES': PAR_NAMES + [f'lncol{k}' for k in more] + (['lnff'] if fill else []),
            'PAR_NAMES_SHORT': PAR_NAMES_SHORT + [f'lN{k}' for k in more] + (['lf'] if fill else []),
            'TEX_LABELS': TEX_LABELS + [rf'$\log(N_{k})$' for k in more] + ([r'$\log(f)$'] if fill else []),
            'TEX_LABELS_WITH_UNITS': TEX_LABELS_WITH_UNITS + [rf'$\log(N_{k}) \ [\mathrm{{cm^{{-2}}}}]$' for k in more]
                                     + ([r'$\log(f)$'] if fill else []),
        }
        bound = {'MIX': self, 'N_MODEL': N, 'MODEL_INFO': self, 'SPECIES': species, 'FILL': fill}
        attrs['Runner'] = type('LteMixRunner', (_MixRunner,), dict(bound))
        attrs['Spectrum'] = type('LteMixSpectrum', (_MixSpectrum,), dict(bound))
        for key, value in attrs.items():
            object.__setattr__(self, key, value)

    n_species = property(lambda self: len(self.species))
    ModelRunner = property(lambda self: self.Runner)
    ModelSpectrum = property(lambda self: self.Spectrum)

    def __setattr__(self, key, value):
        raise AttributeError('an LteMix is immutable')

    def __delattr__(self, key):
        raise AttributeError('an LteMix is immutable')

    def __eq__(self, other):
        if not isinstance(other, LteMix):
            return NotImplemented
        return self.species == other.species and self.fill == other.fill

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return hash(('lte_mix',) + self.species + ((True,) if self.fill else ()))

    def __repr__(self):
        return f'LteMix({", ".join(repr(m.name) for m in self.species)}{", fill=True" if self.fill else ""})'

    @staticmethod
    def lncol_row(k):
        """The parameter (row of a parameter-major vector) that holds the column density of species k."""
        return 2 if k == 0 else 3 + k

    def get_par_names(self, ncomp=None):
        return par_names(self.PAR_NAMES_SHORT, ncomp)

    def predict(self, s, params):
        """Model spectrum of `s` (a `Spectrum` of this mix) for parameter-major `params` (voff, tex, lncol, sigm, lncol2, ...
        and, filled, lnff of every component); result in ``s.get_spec()`` / ``s.loglikelihood``."""
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 1 or params.shape[0] == 0 or params.shape[0] % self.N != 0:
            raise ValueError(f'Invalid parameter vector length: {params.shape}')
        own = params.reshape(self.N, -1)[s._rows]
        s._predict(own.ravel(), own.shape[0])

    model_predict = predict

    def tau_main(self, lines, tex, lncols, sigm):
        """The peak optical depth of every transition of `lines` (an `LteLines`, `LteBand` or `LteBlend`), in its order, each
        with the column density of its own species: `lncols[k]` is species k's.  numpy, one value per transition along the
        first axis, the other arguments broadcasting behind it."""
        check_mix_lines(self.species, [lines], all_species=False)
        if len(lncols) != len(self.species):
            raise ValueError(f'`lncols` takes one column density per species: {len(self.species)}, not {len(lncols)}')
        return np.stack([t.tau_main(tex, lncols[self.species.index(t.molecule)], sigm) for t in transitions_of(lines)])
