"""The likelihood options of a spectra set -- the keywords every runner, `CubeRunner` and a `CubeFitter`'s `runner_kwargs`
share -- in one place: their value checks, the one table of which option goes with which (`RULES`, the Python side of
csrc/nfa_set_rules.h: the same compatibilities, in this side's words) and the record of their normalised values (`Options`,
built by `check_options`).  numpy only: nothing here needs a device, and everything is checked before the first device call.

The options, in the constructors' order (`OPTION_NAMES`):

baseline_order: None, or 0..3 for a polynomial baseline of that degree per spectrum, profiled out of the likelihood in
    closed form (nfa_specset_set_baseline).  null_lnZ is then the baseline-only model's, from the runner's own
    spectra set (the spectra keep the reference's spectrum-alone value), and lnZ - null_lnZ is a Bayes factor of
    baseline-marginalised models.
layered: layered radiative transfer (nfa_specset_set_layered) -- the components are layers along the line of
    sight, component 0 the farthest, and each absorbs those behind it; False: the components are summed.  `predict` of a
    layered runner goes through the runner's own spectra set (`_predict_layered`).  Not for the Gaussian model.
calibration: None, or the fractional 1-sigma uncertainty of the spectra's intensity scales -- a number for all of them or
    one per spectrum, each in [0, 1] -- integrated out of the likelihood in closed form per spectrum
    (nfa_specset_set_calibration); all zeros is None.  null_lnZ is unchanged.
noise_uncertainty: None, or the fractional 1-sigma uncertainty of the spectra's noise levels -- a number for all of them or
    one per spectrum, each in [0, 0.5] -- integrated out of the likelihood in closed form per spectrum
    (nfa_specset_set_noise_uncertainty); all zeros is None.  Goes with everything but a calibration.  null_lnZ
    is then the same function of the parts at p = 0.
correlation: None, or the first two autocorrelations (rho_1, rho_2) of the channel noise along the spectral axis -- a pair
    for all spectra (`HANNING`, `ar1(rho)`) or an array [n_spec, 2] -- for cubes that were smoothed, regridded or oversampled
    (nfa_specset_set_correlation); all zeros is None.  Not with masked channels, a baseline or a calibration.
    null_lnZ is then d^T Q d's, and the spectra's `prefactor` gains -ln det R / 2.
response: None, or the channel response of the spectrometer -- 3 or 5 taps for all spectra (`HANNING_RESPONSE`) or an array
    [n_spec, 3 | 5] -- with which the model is convolved before it meets the data (nfa_specset_set_response);
    the identity is None.  Not with masked channels, a baseline or a calibration.  null_lnZ is unchanged.
templates: None, or a list with one entry per spectrum, each None or an array [T, N_s] of 1..4 fixed shapes on the
    spectrum's channels whose amplitudes are profiled out of the likelihood in closed form together with the baseline
    (nfa_specset_set_templates): `ripple(n_chan, period)` for a standing wave of known period.  Not with a
    calibration, a correlation or a response.  null_lnZ is then the model of baseline and templates alone.
continuum: None, or the brightness temperature Tc >= 0 (K) of a continuum source behind all components -- a number for all
    spectra or one per spectrum (a cube: also [n_pix, n_spec]) -- taken from the continuum map that was subtracted from the
    data: data, not a parameter (nfa_specset_set_continuum).  The line then goes negative wherever J(tex) <
    J(Tcmb) + Tc.  All zeros is None.  Not with the Gaussian model, a calibration, a correlation, a response or templates.
    null_lnZ is unchanged.  `predict` of such a runner goes through the runner's own spectra set, as for `layered`.
robust: None, or the degrees of freedom nu of Student-t channel noise -- a number for all spectra or one per spectrum, each
    0 (that spectrum stays Gaussian) or in [1, 1e6] -- so that an interference spike or an unflagged bad channel costs the
    logarithm of its residual, not its square (nfa_specset_set_robust); 4 is a common choice,
    `cubeio.estimate_tails` measures one.  With a scalar noise, a noise per channel, masked channels, `layered` and filled
    sets; with none of the other likelihood options.  null_lnZ is the same expression at p = 0."""
import numpy as np

OPTION_NAMES = ('baseline_order', 'layered', 'calibration', 'noise_uncertainty', 'correlation', 'response', 'templates',
                'continuum', 'robust')
# the order in which a constructor hands the options that are on to the engine
APPLY_ORDER = ('layered', 'baseline_order', 'calibration', 'correlation', 'response', 'templates', 'noise_uncertainty',
               'continuum', 'robust')
MODEL_GAUSSIAN = 2
BASELINE_MAX = 3          # NFA_BASELINE_MAX
CORR_V_MIN = 0.01         # smallest innovations variance a noise correlation may have
RESP_SUM_TOL = 1e-9       # how far the taps of a channel response may miss the sum 1
TMPL_MAX = 4              # NFA_TMPL_MAX
NOISE_UNCERTAINTY_MAX = 0.5
ROBUST_MIN, ROBUST_MAX = 1.0, 1e6


# ---- the value of every option: shape, range, one per spectrum; "all zeros / the identity is None" ----------------------
def check_baseline_order(order):
    """`baseline_order` of a runner: None (or -1) for no baseline, else an integer 0..BASELINE_MAX; ValueError otherwise."""
    if order is None:
        return None
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)):
        raise ValueError(f'baseline_order must be None or an integer in -1..{BASELINE_MAX}, not {order!r}')
    order = int(order)
    if not -1 <= order <= BASELINE_MAX:
        raise ValueError(f'baseline_order must be None or an integer in -1..{BASELINE_MAX}, not {order}')
    return None if order == -1 else order


def check_layered(layered, model=None):
    """`layered` as a bool; ValueError for anything but True / False, and for the Gaussian model, which has no optical
    depth.  Needs no device."""
    if not isinstance(layered, (bool, np.bool_)):
        raise ValueError('`layered` is True or False: whether a component absorbs the components behind it')
    if layered and model is not None and int(model) == MODEL_GAUSSIAN:
        raise ValueError('the Gaussian model has no optical depth: its components cannot absorb one another (`layered`)')
    return bool(layered)


def _per_spectrum(val, n_spec, what, in_range):
    """A number for all `n_spec` spectra, or one per spectrum, every one finite and `in_range`: None where none is > 0, else
    float64 [n_spec] -- the value of `calibration`, `noise_uncertainty` and `robust`."""
    if val is None:
        return None
    is_num = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    if is_num(val):
        vals = [val] * (1 if n_spec is None else int(n_spec))
    elif isinstance(val, np.ndarray) and val.ndim == 1 and val.dtype.kind in 'iuf':
        vals = list(val)
    elif isinstance(val, (list, tuple)) and all(is_num(v) for v in val):
        vals = list(val)
    else:
        raise ValueError(f'{what}, not {val!r}')
    if not is_num(val) and n_spec is not None and len(vals) != int(n_spec):
        raise ValueError(f'{what}: {len(vals)} values for {int(n_spec)} spectra')
    out = np.array(vals, dtype=np.float64)
    if out.size == 0 or not np.all(np.isfinite(out)) or not np.all(in_range(out)):
        raise ValueError(f'{what}, not {val!r}')
    return out if np.any(out > 0.0) else None


def _calibration(cal, n_spec=None):
    return _per_spectrum(cal, n_spec, 'calibration must be None, a number in [0, 1] or one such number per spectrum',
                         lambda v: (v >= 0.0) & (v <= 1.0))


def _noise_uncertainty(f, n_spec=None):
    return _per_spectrum(f, n_spec, 'noise uncertainty (noise_uncertainty) must be None, a number in [0, 0.5] or one such number '
                         'per spectrum', lambda v: (v >= 0.0) & (v <= NOISE_UNCERTAINTY_MAX))


def _robust(nu, n_spec=None):
    return _per_spectrum(nu, n_spec, 'robust must be None, degrees of freedom in [1, 1e6] (0: Gaussian) or one such number per '
                         'spectrum', lambda v: (v == 0.0) | ((v >= ROBUST_MIN) & (v <= ROBUST_MAX)))


def yule_walker(rho1, rho2):
    """(phi_1, phi_2, v) of the unit-variance AR(2) process whose first two autocorrelations are (rho1, rho2): the
    coefficients and the innovations variance."""
    den = 1.0 - rho1 * rho1
    phi1, phi2 = rho1 * (1.0 - rho2) / den, (rho2 - rho1 * rho1) / den
    return phi1, phi2, 1.0 - phi1 * rho1 - phi2 * rho2


def _correlation(corr, n_spec=None, sizes=None):
    if corr is None:
        return None
    what = 'correlation must be None, a pair (rho_1, rho_2) or an array [n_spec, 2] of such pairs'
    try:
        out = np.array(corr, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'{what}, not {corr!r}') from None
    if isinstance(corr, np.ndarray) and corr.dtype.kind not in 'iuf':
        raise ValueError(f'{what}, not {corr!r}')
    if out.ndim == 1 and out.shape == (2,):
        out = np.tile(out, (1 if n_spec is None else int(n_spec), 1))
    elif out.ndim != 2 or out.shape[1] != 2 or out.shape[0] == 0:
        raise ValueError(f'{what}, not {corr!r}')
    elif n_spec is not None and out.shape[0] != int(n_spec):
        raise ValueError(f'{what}: {out.shape[0]} pairs for {int(n_spec)} spectra')
    if not np.all(np.isfinite(out)):
        raise ValueError(f'{what}: every value finite, not {corr!r}')
    for r1, r2 in out:
        if r1 == 0.0 and r2 == 0.0:
            continue
        if not abs(r1) < 1.0:
            raise ValueError(f'correlation: |rho_1| < 1, not {r1!r}')
        if not 2.0 * r1 * r1 - 1.0 < r2 < 1.0:
            raise ValueError(f'correlation: 2 rho_1^2 - 1 < rho_2 < 1 (a positive definite correlation matrix), not ({r1!r}, {r2!r})')
        if not yule_walker(r1, r2)[2] >= CORR_V_MIN:
            raise ValueError(f'correlation: the innovations variance of ({r1!r}, {r2!r}) is below {CORR_V_MIN}: the noise is '
                             'nearly determined by its neighbours')
    if not np.any(out != 0.0):
        return None
    if sizes is not None and np.any(np.asarray(sizes) < 4):
        raise ValueError('a noise correlation needs spectra of 4 channels and more')
    return np.ascontiguousarray(out)


def _response(resp, n_spec=None, sizes=None):
    if resp is None:
        return None
    what = 'response must be None, 3 or 5 taps (h_-T .. h_T) or an array [n_spec, 3 | 5] of such taps'
    if isinstance(resp, (list, tuple)) and len(resp) > 0 and all(isinstance(r, (list, tuple, np.ndarray)) and np.ndim(r) == 1 and
                                                                 len(r) in (3, 5) for r in resp):
        resp = [[0.0, *r, 0.0] if len(r) == 3 else list(r) for r in resp]      # responses of three and of five taps side by side
    try:
        out = np.array(resp, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'{what}, not {resp!r}') from None
    if isinstance(resp, np.ndarray) and resp.dtype.kind not in 'iuf':
        raise ValueError(f'{what}, not {resp!r}')
    if out.ndim == 1 and out.shape[0] in (3, 5):
        out = np.tile(out, (1 if n_spec is None else int(n_spec), 1))
    elif out.ndim != 2 or out.shape[1] not in (3, 5) or out.shape[0] == 0:
        raise ValueError(f'{what}, not {resp!r}')
    elif n_spec is not None and out.shape[0] != int(n_spec):
        raise ValueError(f'{what}: {out.shape[0]} responses for {int(n_spec)} spectra')
    if not np.all(np.isfinite(out)):
        raise ValueError(f'{what}: every tap finite, not {resp!r}')
    if out.shape[1] == 3:
        out = np.pad(out, ((0, 0), (1, 1)))
    for h in out:
        if not abs(float(np.sum(h)) - 1.0) <= RESP_SUM_TOL:
            raise ValueError(f'channel response: the taps sum to 1 (it conserves the integrated intensity), not {float(np.sum(h))!r}')
        if not h[2] > 0.0:
            raise ValueError(f'channel response: the central tap is > 0, not {float(h[2])!r}')
    if np.all(out == np.array([0.0, 0.0, 1.0, 0.0, 0.0])):
        return None
    if sizes is not None and np.any(np.asarray(sizes) < 4):
        raise ValueError('a channel response needs spectra of 4 channels and more')
    return np.ascontiguousarray(out)


def _templates(tmpl, n_spec=None, sizes=None):
    if tmpl is None:
        return None
    what = 'templates must be None or a list with one entry per spectrum, each None or an array [T, n_chan] of 1..4 templates'
    if isinstance(tmpl, np.ndarray) and tmpl.ndim in (1, 2) and tmpl.dtype.kind in 'iuf' and n_spec in (None, 1):
        tmpl = [tmpl]                                         # one spectrum: its array alone
    if not isinstance(tmpl, (list, tuple)) or len(tmpl) == 0:
        raise ValueError(f'{what}, not {tmpl!r}')
    if n_spec is not None and len(tmpl) != int(n_spec):
        raise ValueError(f'{what}: {len(tmpl)} entries for {int(n_spec)} spectra')
    out = []
    for k, t in enumerate(tmpl):
        if t is None:
            out.append(None)
            continue
        try:
            a = np.array(t, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f'{what}; spectrum {k}: {t!r}') from None
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[1] == 0:
            raise ValueError(f'{what}; spectrum {k} has shape {a.shape}')
        if a.shape[0] == 0:
            out.append(None)
            continue
        if a.shape[0] > TMPL_MAX:
            raise ValueError(f'nuisance templates: at most {TMPL_MAX} per spectrum, not {a.shape[0]} (spectrum {k})')
        if sizes is not None and a.shape[1] != int(sizes[k]):
            raise ValueError(f'nuisance templates: spectrum {k} has {int(sizes[k])} channels, its templates {a.shape[1]}')
        if not np.all(np.isfinite(a)):
            raise ValueError(f'nuisance templates: every value finite (spectrum {k})')
        if np.any(np.all(a == 0.0, axis=1)):
            raise ValueError(f'nuisance templates: a template is zero over its whole spectrum (spectrum {k})')
        out.append(np.ascontiguousarray(a))
    return None if all(a is None for a in out) else out


def _continuum(tc, n_spec=None, n_pix=None, model=None):
    if tc is None:
        return None
    what = ('continuum must be None, a brightness temperature >= 0 in K, one per spectrum'
            + (' or an array [n_pix, n_spec]' if n_pix is not None else ''))
    if isinstance(tc, (bool, np.bool_)) or (isinstance(tc, np.ndarray) and tc.dtype.kind not in 'iuf'):
        raise ValueError(f'{what}, not {tc!r}')
    try:
        out = np.array(tc, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'{what}, not {tc!r}') from None
    if out.ndim == 0:
        out = np.full(1 if n_spec is None else int(n_spec), float(out))
    elif out.ndim == 1 and out.size > 0:
        if n_spec is not None and out.shape[0] != int(n_spec):
            raise ValueError(f'{what}: {out.shape[0]} values for {int(n_spec)} spectra')
    elif out.ndim == 2 and n_pix is not None and out.size > 0:
        if out.shape[0] != int(n_pix) or (n_spec is not None and out.shape[1] != int(n_spec)):
            raise ValueError(f'{what}: shape {out.shape} for {int(n_pix)} pixels of {n_spec} spectra')
    else:
        raise ValueError(f'{what}, not an array of shape {out.shape}')
    if not np.all(np.isfinite(out)) or np.any(out < 0.0):
        raise ValueError(f'{what}: every value finite and >= 0, not {tc!r}')
    if not np.any(out > 0.0):
        return None
    if n_pix is not None and out.ndim == 1:
        out = np.tile(out, (int(n_pix), 1))
    if model is not None and int(model) == MODEL_GAUSSIAN:
        raise ValueError('the Gaussian model has no optical depth: its components cannot absorb a continuum background (continuum)')
    return np.ascontiguousarray(out)


def normalise(name, value, n_spec=None, sizes=None, model=None, n_pix=None):
    """The value check of option `name` alone: `value` in the form the engine's setter takes, None (False for `layered`)
    where the option is off; ValueError otherwise.  An option's own conditions are part of it: spectra of 4 channels and more
    (`sizes`) for a correlation and a response, no Gaussian `model` for `layered` and a continuum, [n_pix, n_spec] for a
    cube's continuum alone."""
    if name == 'baseline_order':
        return check_baseline_order(value)
    if name == 'layered':
        return check_layered(value, model)
    if name == 'continuum':
        return _continuum(value, n_spec, n_pix, model)
    if name in ('correlation', 'response', 'templates'):
        return {'correlation': _correlation, 'response': _response, 'templates': _templates}[name](value, n_spec, sizes)
    return {'calibration': _calibration, 'noise_uncertainty': _noise_uncertainty, 'robust': _robust}[name](value, n_spec)


def is_set(value):
    """Whether a normalised value switches its option on: not None, and not `layered`'s False."""
    return value is not None and value is not False


# ---- which option goes with which -------------------------------------------------------------------------------------
_NUNC_CALIB = 'a noise uncertainty does not go with a calibration uncertainty (calibration): a calibrated spectrum\'s part is no chi^2'
_ROB_NOT_WITH = 'a robust likelihood (robust) does not go with {}: under Student-t noise no linear nuisance has a closed form and a part is no chi^2'
_ROB = {'baseline_order': 'a baseline (baseline_order)', 'calibration': 'a calibration uncertainty (calibration)',
        'correlation': 'a noise correlation (correlation)', 'response': 'a channel response (response)',
        'templates': 'nuisance templates (templates)', 'noise_uncertainty': 'a noise uncertainty (noise_uncertainty)',
        'continuum': 'a continuum background (continuum)'}

# (takes, has, message): a set that has `has` -- one of OPTION_NAMES, or 'masked' channels -- does not take `takes`.  The rows
# of one `takes` stand in the order in which they are asked: the first that applies is the refusal.
RULES = (
    ('baseline_order', 'response', 'a baseline does not go with a channel response (response)'),
    ('baseline_order', 'correlation', 'a baseline does not go with a noise correlation (correlation)'),
    ('baseline_order', 'robust', _ROB_NOT_WITH.format(_ROB['baseline_order'])),
    ('calibration', 'noise_uncertainty', _NUNC_CALIB),
    ('calibration', 'response', 'a calibration uncertainty does not go with a channel response (response)'),
    ('calibration', 'correlation', 'a calibration uncertainty does not go with a noise correlation (correlation)'),
    ('calibration', 'templates', 'a calibration uncertainty does not go with nuisance templates (templates)'),
    ('calibration', 'continuum', 'a calibration uncertainty does not go with a continuum background (continuum)'),
    ('calibration', 'robust', _ROB_NOT_WITH.format(_ROB['calibration'])),
    ('noise_uncertainty', 'calibration', _NUNC_CALIB),
    ('noise_uncertainty', 'robust', _ROB_NOT_WITH.format(_ROB['noise_uncertainty'])),
    ('correlation', 'masked', 'a noise correlation does not go with masked channels (channel noise inf)'),
    ('correlation', 'baseline_order', 'a noise correlation does not go with a baseline (baseline_order)'),
    ('correlation', 'calibration', 'a noise correlation does not go with a calibration uncertainty (calibration)'),
    ('correlation', 'templates', 'a noise correlation does not go with nuisance templates (templates)'),
    ('correlation', 'continuum', 'a noise correlation does not go with a continuum background (continuum)'),
    ('correlation', 'robust', _ROB_NOT_WITH.format(_ROB['correlation'])),
    ('response', 'masked', 'a channel response does not go with masked channels (channel noise inf)'),
    ('response', 'baseline_order', 'a channel response does not go with a baseline (baseline_order)'),
    ('response', 'calibration', 'a channel response does not go with a calibration uncertainty (calibration)'),
    ('response', 'templates', 'a channel response does not go with nuisance templates (templates)'),
    ('response', 'continuum', 'a channel response does not go with a continuum background (continuum)'),
    ('response', 'robust', _ROB_NOT_WITH.format(_ROB['response'])),
    ('templates', 'calibration', 'nuisance templates do not go with a calibration uncertainty (calibration)'),
    ('templates', 'correlation', 'nuisance templates do not go with a noise correlation (correlation)'),
    ('templates', 'response', 'nuisance templates do not go with a channel response (response)'),
    ('templates', 'continuum', 'nuisance templates do not go with a continuum background (continuum)'),
    ('templates', 'robust', _ROB_NOT_WITH.format(_ROB['templates'])),
    ('continuum', 'calibration', 'a continuum background does not go with a calibration uncertainty (calibration)'),
    ('continuum', 'correlation', 'a continuum background does not go with a noise correlation (correlation)'),
    ('continuum', 'response', 'a continuum background does not go with a channel response (response)'),
    ('continuum', 'templates', 'a continuum background does not go with nuisance templates (templates)'),
    ('continuum', 'robust', _ROB_NOT_WITH.format(_ROB['continuum'])),
    *(('robust', has, _ROB_NOT_WITH.format(_ROB[has])) for has in ('baseline_order', 'calibration', 'correlation', 'response',
                                                                  'templates', 'noise_uncertainty', 'continuum')),
)


MODEL_GRID = 5
# A set of the excitation-grid model (nestfit_amd.excitation) runs a kernel side of its own, and a side is
# exclusive: the options of the other sides, and a calibration, are refused by the model, in the engine's words.
_GRID_TAKES_NO = {'calibration': 'calibration uncertainty', 'correlation': 'noise correlation', 'response': 'channel response',
                  'templates': 'nuisance templates', 'continuum': 'continuum background', 'robust': 'robust likelihood'}


def model_refusal(takes, model):
    """Why a set of `model` does not take option `takes` whatever else it has, or None: the excitation-grid model's six."""
    if model is not None and int(model) == MODEL_GRID and takes in _GRID_TAKES_NO:
        return 'a set of the excitation-grid model takes no ' + _GRID_TAKES_NO[takes]
    return None


def refusal(takes, has):
    """Why a set that has the features `has` (names of OPTION_NAMES and 'masked') does not take option `takes`, or None."""
    return next((why for t, h, why in RULES if t == takes and h in has), None)


def is_on(name, value):
    """Whether `value`, as a caller gives it to a `check_*` function beside the option it checks (raw or normalised),
    switches feature `name` on."""
    if name == 'masked':
        return bool(value)
    if name == 'baseline_order':
        return value is not None and value != -1
    if name in ('calibration', 'continuum'):
        return value is not None and bool(np.any(np.asarray(value, dtype=np.float64) > 0.0))
    if name == 'templates':
        return value is not None and any(t is not None for t in value)
    return normalise(name, value) is not None               # (all zeros, the identity: off)


def _checked(takes, value, **others):
    """`value`, the normalised value of option `takes`, after asking the table about the other features the caller named (as
    given or normalised); ValueError with the first refusal."""
    if is_set(value):
        for t, has, why in RULES:
            if t == takes and has in others and is_on(has, others[has]):
                raise ValueError(why)
    return value


def check_calibration(cal, n_spec=None):
    """`calibration` of a runner: the fractional 1-sigma uncertainty of every spectrum's intensity scale.  None
    for none; a number applies to all `n_spec` spectra; else one value per spectrum.  Every value is a finite number in
    [0, 1]; all zeros is None.  Returns None or a float64 array (of n_spec values when n_spec is given); ValueError
    otherwise.  Needs no device."""
    return _calibration(cal, n_spec)


def check_noise_uncertainty(f, n_spec=None, calibration=None):
    """`noise_uncertainty` of a runner: the fractional 1-sigma uncertainty of every spectrum's noise level.
    None for none; a number applies to all `n_spec` spectra; else one value per spectrum.  Every value is a finite number
    in [0, 0.5] (above that the first-order relation a = 1 / (4 f^2) means nothing); all zeros is None.  Not with a
    calibration uncertainty (`calibration`).  Returns None or a float64 array (of n_spec values when n_spec is given);
    ValueError otherwise.  Needs no device."""
    return _checked('noise_uncertainty', _noise_uncertainty(f, n_spec), calibration=calibration)


def check_correlation(corr, n_spec=None, sizes=None, masked=False, baseline_order=None, calibration=None):
    """`correlation` of a runner: the first two autocorrelations (rho_1, rho_2) of the channel noise along the spectral axis
    (DESIGN 4.13).  None for none; a pair applies to all `n_spec` spectra; an array [n_spec, 2] gives one pair per spectrum
    (a one-dimensional value is always ONE pair).  Every pair is finite with |rho_1| < 1, 2 rho_1^2 - 1 < rho_2 < 1 and an
    innovations variance v >= 0.01, or (0, 0) for white noise; all zeros is None.  A correlation goes with neither a masked
    channel (`masked`), a baseline (`baseline_order`) nor a calibration uncertainty (`calibration`), and needs spectra of 4
    channels and more (`sizes`).  Returns None or a float64 array [n_spec, 2] ([1, 2] without n_spec); ValueError otherwise.
    Needs no device."""
    return _checked('correlation', _correlation(corr, n_spec, sizes), masked=masked, baseline_order=baseline_order,
                    calibration=calibration)


def check_response(resp, n_spec=None, sizes=None, masked=False, baseline_order=None, calibration=None):
    """`response` of a runner: the channel response of the spectrometer, an odd number of taps, 3 or 5, (h_-T .. h_0 .. h_T)
    in units of channels; the model that meets the data is sum_k h_k p_{j+k}.  None for none; one response
    applies to all `n_spec` spectra; an array [n_spec, 3 | 5] gives one per spectrum (a one-dimensional value is always ONE
    response).  Every tap is finite, the taps sum to 1 within 1e-9 and h_0 > 0; (0, 1, 0) is an unfiltered spectrum, and
    the identity everywhere is None.  A response goes with neither a masked channel (`masked`), a baseline
    (`baseline_order`) nor a calibration uncertainty (`calibration`), and needs spectra of 4 channels and more (`sizes`).
    Returns None or a float64 array [n_spec, 5] ([1, 5] without n_spec), three taps padded with zero ends; ValueError
    otherwise.  Needs no device."""
    return _checked('response', _response(resp, n_spec, sizes), masked=masked, baseline_order=baseline_order, calibration=calibration)


def check_templates(tmpl, n_spec=None, sizes=None, calibration=None, correlation=None, response=None):
    """`templates` of a runner: fixed shapes on the channel grid, known up to an amplitude, that are profiled out of the
    likelihood with the baseline.  None for none; else a list with one entry per spectrum, each None or an
    array [T, N_s] of 1 <= T <= 4 templates over the spectrum's N_s channels (one row may be given as a 1-D array).  Every
    value is finite and no template is zero over its whole spectrum; all entries None is None.  Nuisance templates go with
    neither a calibration uncertainty, a noise correlation nor a channel response.  Returns None or a list of n_spec entries,
    None or float64 [T, N_s]; ValueError otherwise.  Needs no device."""
    return _checked('templates', _templates(tmpl, n_spec, sizes), calibration=calibration, correlation=correlation, response=response)


def check_continuum(tc, n_spec=None, n_pix=None, model=None, calibration=None, correlation=None, response=None, templates=None):
    """`continuum` of a runner: the brightness temperature Tc >= 0 (K, on the data's scale) of a continuum source behind all
    components, per spectrum -- data of the continuum map that was subtracted, not a parameter.  None for none;
    a number applies to all spectra (and pixels); one value per spectrum, [n_spec]; with `n_pix` given (a cube) also
    [n_pix, n_spec].  Every value is finite and >= 0; all zeros is None.  A continuum goes with neither the Gaussian model
    (`model`: no optical depth), a calibration uncertainty, a noise correlation, a channel response nor nuisance templates.
    Returns None or a float64 array [n_spec] ([n_pix, n_spec] with n_pix; [1] for a number without n_spec); ValueError
    otherwise.  Needs no device."""
    return _checked('continuum', _continuum(tc, n_spec, n_pix, model), calibration=calibration, correlation=correlation,
                    response=response, templates=templates)


def check_robust(nu, n_spec=None, baseline_order=None, calibration=None, correlation=None, response=None, templates=None,
                 noise_uncertainty=None, continuum=None):
    """`robust` of a runner: the degrees of freedom nu of the Student-t channel noise of every spectrum.  None
    for none; a number applies to all `n_spec` spectra; else one value per spectrum.  Every value is finite and either 0
    (that spectrum stays Gaussian) or in [1, 1e6] (beyond, the value is the Gaussian one within 1e-6: leave it out); all
    zeros is None.  A robust likelihood goes with none of a baseline, a calibration uncertainty, a noise correlation, a
    channel response, nuisance templates, a noise uncertainty and a continuum background.  Returns None or a float64 array
    (of n_spec values when n_spec is given); ValueError otherwise.  Needs no device."""
    nu = _robust(nu, n_spec)
    if nu is not None:
        baseline_order = check_baseline_order(baseline_order)
    return _checked('robust', nu, baseline_order=baseline_order, calibration=calibration, correlation=correlation, response=response,
                    templates=templates, noise_uncertainty=noise_uncertainty, continuum=continuum)


# ---- the record ---------------------------------------------------------------------------------------------------------
class Options:
    """The nine options of one set, normalised: None (`layered`: False) where an option is off."""
    __slots__ = OPTION_NAMES

    def __init__(self):
        for name in OPTION_NAMES:
            setattr(self, name, False if name == 'layered' else None)

    def has(self, masked=False):
        """The names of the options that are on, and 'masked' for a set with masked channels: `refusal`'s `has`."""
        on = {name for name in OPTION_NAMES if is_set(getattr(self, name))}
        return on | {'masked'} if masked else on


def refuse_unknown(options, caller):
    """The TypeError of a call of `caller` (a function's qualified name) with a keyword that is none of OPTION_NAMES, in the
    words of Python's own: the constructors take the options as `**options`."""
    for key in options:
        if key not in OPTION_NAMES:
            raise TypeError(f"{caller}() got an unexpected keyword argument '{key}'")


def check_options(options, n_spec, sizes=None, masked=False, model=None, n_pix=None, caller=None):
    """The `Options` of a mapping of the keywords as a caller gave them (any subset of OPTION_NAMES), for `n_spec` spectra of
    `sizes` channels, with or without `masked` channels, of `model`; `n_pix`: of a cube.  Every option in OPTION_NAMES order:
    its value check, then, where it is on, the table against the options before it and the masked channels -- so the first
    thing wrong in that order is the one named, ValueError.  `caller`: the name of a function whose keywords these are, which
    takes no others (`refuse_unknown`); None: the other keys are somebody else's."""
    if caller is not None:
        refuse_unknown(options, caller)
    out = Options()
    for name in OPTION_NAMES:
        if name in options:
            value = normalise(name, options[name], n_spec, sizes, model, n_pix)
            if is_set(value):
                why = model_refusal(name, model) or refusal(name, out.has(masked))
                if why is not None:
                    raise ValueError(why)
            setattr(out, name, value)
    return out
