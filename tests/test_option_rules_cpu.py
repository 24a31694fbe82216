"""Which likelihood option goes with which is one table on the Python side, nestfit_amd/_options.py (`RULES`), as
csrc/nfa_set_rules.h is the engine's.  Before the table every `check_*` function and every `_SpecSet.set_*` method carried its
own chain of `if`s; this test holds `check_options` and `refusal` to those chains, transcribed below with their messages one
`if` per line in their order, for every subset of the ten features (1024) and every setter.  numpy only: no engine is loaded;
the setters run against a stand-in for the engine's library that accepts every call."""
import itertools
import types

import numpy as np
import pytest

from nestfit_amd import _options as opt

FEATURES = ('masked', 'baseline_order', 'calibration', 'noise_uncertainty', 'correlation', 'response', 'templates', 'continuum',
            'robust', 'layered')
N_CHAN = 8
# the smallest valid value that switches each option on, for one spectrum of 8 channels, and values that leave it off
ON = {'baseline_order': 0, 'layered': True, 'calibration': 0.1, 'noise_uncertainty': 0.1, 'correlation': (0.5, 0.25),
      'response': (0.25, 0.5, 0.25), 'templates': [np.ones((1, N_CHAN))], 'continuum': 1.0, 'robust': 4}
OFF = {'baseline_order': (None, -1), 'layered': (False,), 'calibration': (None, 0.0, [0.0]), 'noise_uncertainty': (None, 0, [0.0]),
       'correlation': (None, (0.0, 0.0), np.zeros((1, 2))), 'response': (None, (0, 1, 0), (0, 0, 1, 0, 0)),
       'templates': (None, [None], [np.zeros((0, N_CHAN))]), 'continuum': (None, 0.0, [0.0]), 'robust': (None, 0, [0.0])}
SETTERS = {'baseline_order': 'set_baseline', 'calibration': 'set_calibration', 'noise_uncertainty': 'set_noise_uncertainty',
           'correlation': 'set_correlation', 'response': 'set_response', 'templates': 'set_templates', 'continuum': 'set_continuum',
           'robust': 'set_robust'}

NUNC_CALIB = "a noise uncertainty does not go with a calibration uncertainty (calibration): a calibrated spectrum's part is no chi^2"
rob = ('a robust likelihood (robust) does not go with {}: under Student-t noise no linear nuisance has a closed form and a part is '
       'no chi^2').format


def subsets():
    for k in range(len(FEATURES) + 1):
        for s in itertools.combinations(FEATURES, k):
            yield frozenset(s)


def constructor_chain(s):
    """The cross-checks of the six `check_*` functions as `EngineRunner._setup` and `CubeRunner.__init__` called them, in that
    order: the first `if` that applies is what the constructor raised."""
    if 'noise_uncertainty' in s:                # check_noise_uncertainty(f, n, calibration)
        if 'calibration' in s: return NUNC_CALIB
    if 'correlation' in s:                      # check_correlation(corr, n, sizes, masked, baseline_order, calibration)
        if 'masked' in s: return 'a noise correlation does not go with masked channels (channel noise inf)'
        if 'baseline_order' in s: return 'a noise correlation does not go with a baseline (baseline_order)'
        if 'calibration' in s: return 'a noise correlation does not go with a calibration uncertainty (calibration)'
    if 'response' in s:                         # check_response(resp, n, sizes, masked, baseline_order, calibration)
        if 'masked' in s: return 'a channel response does not go with masked channels (channel noise inf)'
        if 'baseline_order' in s: return 'a channel response does not go with a baseline (baseline_order)'
        if 'calibration' in s: return 'a channel response does not go with a calibration uncertainty (calibration)'
    if 'templates' in s:                        # check_templates(tmpl, n, sizes, calibration, correlation, response)
        if 'calibration' in s: return 'nuisance templates do not go with a calibration uncertainty (calibration)'
        if 'correlation' in s: return 'nuisance templates do not go with a noise correlation (correlation)'
        if 'response' in s: return 'nuisance templates do not go with a channel response (response)'
    if 'continuum' in s:                        # check_continuum(tc, n, n_pix, model, calibration, correlation, response, templates)
        if 'calibration' in s: return 'a continuum background does not go with a calibration uncertainty (calibration)'
        if 'correlation' in s: return 'a continuum background does not go with a noise correlation (correlation)'
        if 'response' in s: return 'a continuum background does not go with a channel response (response)'
        if 'templates' in s: return 'a continuum background does not go with nuisance templates (templates)'
    if 'robust' in s:                           # check_robust(nu, n, baseline_order, ..., noise_uncertainty, continuum)
        if 'baseline_order' in s: return rob('a baseline (baseline_order)')
        if 'calibration' in s: return rob('a calibration uncertainty (calibration)')
        if 'correlation' in s: return rob('a noise correlation (correlation)')
        if 'response' in s: return rob('a channel response (response)')
        if 'templates' in s: return rob('nuisance templates (templates)')
        if 'noise_uncertainty' in s: return rob('a noise uncertainty (noise_uncertainty)')
        if 'continuum' in s: return rob('a continuum background (continuum)')
    return None


def setter_chain(has, takes):
    """The eight `_SpecSet.set_*` chains as they stood, the `check_*` call's part first: a set that has `has` is asked to
    switch `takes` on."""
    if takes == 'robust':                       # set_robust
        if 'baseline_order' in has: return rob('a baseline (baseline_order)')
        if 'calibration' in has: return rob('a calibration uncertainty (calibration)')
        if 'correlation' in has: return rob('a noise correlation (correlation)')
        if 'response' in has: return rob('a channel response (response)')
        if 'templates' in has: return rob('nuisance templates (templates)')
        if 'noise_uncertainty' in has: return rob('a noise uncertainty (noise_uncertainty)')
        if 'continuum' in has: return rob('a continuum background (continuum)')
    if takes == 'continuum':                    # set_continuum
        if 'calibration' in has: return 'a continuum background does not go with a calibration uncertainty (calibration)'
        if 'correlation' in has: return 'a continuum background does not go with a noise correlation (correlation)'
        if 'response' in has: return 'a continuum background does not go with a channel response (response)'
        if 'templates' in has: return 'a continuum background does not go with nuisance templates (templates)'
        if 'robust' in has: return rob('a continuum background (continuum)')
    if takes == 'templates':                    # set_templates
        if 'calibration' in has: return 'nuisance templates do not go with a calibration uncertainty (calibration)'
        if 'correlation' in has: return 'nuisance templates do not go with a noise correlation (correlation)'
        if 'response' in has: return 'nuisance templates do not go with a channel response (response)'
        if 'continuum' in has: return 'nuisance templates do not go with a continuum background (continuum)'
        if 'robust' in has: return rob('nuisance templates (templates)')
    if takes == 'response':                     # set_response
        if 'masked' in has: return 'a channel response does not go with masked channels (channel noise inf)'
        if 'baseline_order' in has: return 'a channel response does not go with a baseline (baseline_order)'
        if 'calibration' in has: return 'a channel response does not go with a calibration uncertainty (calibration)'
        if 'templates' in has: return 'a channel response does not go with nuisance templates (templates)'
        if 'continuum' in has: return 'a channel response does not go with a continuum background (continuum)'
        if 'robust' in has: return rob('a channel response (response)')
    if takes == 'correlation':                  # set_correlation
        if 'masked' in has: return 'a noise correlation does not go with masked channels (channel noise inf)'
        if 'baseline_order' in has: return 'a noise correlation does not go with a baseline (baseline_order)'
        if 'calibration' in has: return 'a noise correlation does not go with a calibration uncertainty (calibration)'
        if 'templates' in has: return 'a noise correlation does not go with nuisance templates (templates)'
        if 'continuum' in has: return 'a noise correlation does not go with a continuum background (continuum)'
        if 'robust' in has: return rob('a noise correlation (correlation)')
    if takes == 'noise_uncertainty':            # set_noise_uncertainty
        if 'calibration' in has: return NUNC_CALIB
        if 'robust' in has: return rob('a noise uncertainty (noise_uncertainty)')
    if takes == 'calibration':                  # set_calibration
        if 'noise_uncertainty' in has: return NUNC_CALIB
        if 'response' in has: return 'a calibration uncertainty does not go with a channel response (response)'
        if 'correlation' in has: return 'a calibration uncertainty does not go with a noise correlation (correlation)'
        if 'templates' in has: return 'a calibration uncertainty does not go with nuisance templates (templates)'
        if 'continuum' in has: return 'a calibration uncertainty does not go with a continuum background (continuum)'
        if 'robust' in has: return rob('a calibration uncertainty (calibration)')
    if takes == 'baseline_order':               # set_baseline
        if 'response' in has: return 'a baseline does not go with a channel response (response)'
        if 'correlation' in has: return 'a baseline does not go with a noise correlation (correlation)'
        if 'robust' in has: return rob('a baseline (baseline_order)')
    return None


def raised(call, *args, **kwargs):
    try:
        call(*args, **kwargs)
    except ValueError as e:
        return str(e)
    return None


def test_the_names_and_their_order():
    assert opt.OPTION_NAMES == ('baseline_order', 'layered', 'calibration', 'noise_uncertainty', 'correlation', 'response',
                                'templates', 'continuum', 'robust')
    assert sorted(opt.APPLY_ORDER) == sorted(opt.OPTION_NAMES)
    assert {t for t, _, _ in opt.RULES} <= set(opt.OPTION_NAMES) and {h for _, h, _ in opt.RULES} <= set(FEATURES)
    assert len({(t, h) for t, h, _ in opt.RULES}) == len(opt.RULES) == 40       # 19 pairs from both sides, a mask from one


def test_every_subset_of_the_features_is_refused_as_the_constructors_chains_refused_it():
    """1024 subsets through `check_options`: the transcription's first message character for character, or no error and a
    record that holds exactly the subset."""
    n_refused = 0
    for s in subsets():
        kw = {name: ON[name] for name in s if name != 'masked'}
        want = constructor_chain(s)
        assert raised(opt.check_options, kw, 1, [N_CHAN], 'masked' in s, 0) == want, sorted(s)
        n_refused += want is not None
        if want is None:
            assert opt.check_options(kw, 1, [N_CHAN], 'masked' in s, 0).has('masked' in s) == s
    assert 0 < n_refused < 1024
    # what is off refuses nothing and is refused nothing: every option at each of its neutral values, together
    for k in range(3):
        off = {name: values[min(k, len(values) - 1)] for name, values in OFF.items()}
        assert opt.check_options(off, 1, [N_CHAN], True, 0).has() == frozenset()
    with pytest.raises(TypeError, match=r"^Runner\.__init__\(\) got an unexpected keyword argument 'nonsense'$"):
        opt.check_options({'robust': 4, 'nonsense': 1}, 1, caller='Runner.__init__')
    assert opt.check_options({'robust': 4, 'ncomp': 2}, 1).robust[0] == 4.0      # no caller named: the other keys are not its


def test_the_constructors_refuse_a_keyword_they_never_took():
    """The runners take the options as `**options`; what is none of the nine is still the TypeError of a function that has no
    such parameter, in Python's words with the name of the function that was called, and before anything else is looked at:
    `nonsense=` and `rest_freqs=` for every runner, `cold=` and `lte=` for every runner but AmmoniaRunner.  No device: the
    spectra are never touched."""
    import nestfit_amd as na
    from nestfit_amd.cube import CubeRunner
    mix = na.LteMix([na.Molecule('mol', [5.0, 10.0], [1.0, 2.0])])
    one = types.SimpleNamespace(rest_freq=1e11, size=N_CHAN, noise=0.1)
    runners = ((na.AmmoniaRunner, 'AmmoniaRunner', []), (na.DiazenyliumRunner, 'DiazenyliumRunner', []),
               (na.GaussianRunner, 'GaussianRunner', one), (na.HyperfineRunner, 'HyperfineRunner', []),
               (na.LteRunner, 'LteRunner', []), (mix.Runner, '_MixRunner', []))
    for cls, name, spectra in runners:
        for key in ('nonsense', 'rest_freqs') + (() if cls is na.AmmoniaRunner else ('cold', 'lte')):
            with pytest.raises(TypeError) as e:
                cls(spectra, None, ncomp=2, baseline_order=7, **{key: True})
            assert str(e.value) == f"{name}.__init__() got an unexpected keyword argument '{key}'", (name, key)
    x = np.linspace(1.0e11, 1.0001e11, N_CHAN)
    with pytest.raises(TypeError) as e:
        CubeRunner([x], [1], np.zeros((1, N_CHAN)), np.full((1, 1), 0.1), None, nonsense=True)
    assert str(e.value) == "CubeRunner.__init__() got an unexpected keyword argument 'nonsense'"
    with pytest.raises(TypeError, match='positional'):      # the options are keywords: none slips into another's place
        CubeRunner([x], [1], np.zeros((1, N_CHAN)), np.full((1, 1), 0.1), None, 1, False, False, 0, None, 1)


@pytest.fixture
def fake_set(monkeypatch):
    """`_SpecSet` objects of one spectrum whose engine accepts every call: what remains of a setter is its Python part."""
    from nestfit_amd import _ffi, _model
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *args: calls.append(name) or 0
    monkeypatch.setattr(_ffi, 'load', lambda: Lib())

    def make(has):
        ss = _model._SpecSet.__new__(_model._SpecSet)
        ss.__dict__.update(handle=None, n_spec=1, n_pix=1, model=0, sizes=np.array([N_CHAN]), chan_tot=N_CHAN,
                           offsets=np.array([0, N_CHAN]), masked='masked' in has, options=opt.Options())
        for name in has - {'masked'}:
            setattr(ss.options, name, opt.normalise(name, ON[name], 1, [N_CHAN]))
        return ss
    return types.SimpleNamespace(make=make, calls=calls)


def test_every_set_and_every_setter_is_refused_as_the_setters_chains_refused_it(fake_set):
    """1024 states x 8 setters: `refusal` gives the chain's message or None, the setter raises it (and leaves the record as it
    was) or stores the value; the same setter with a value that is off is never refused."""
    n_refused = 0
    for has in subsets():
        for takes, setter in SETTERS.items():
            want = setter_chain(has - {takes}, takes)       # (a setter replaces what its own call gave)
            assert opt.refusal(takes, has) == want, (sorted(has), takes)
            n_refused += want is not None
            ss = fake_set.make(has)
            del fake_set.calls[:]
            assert raised(getattr(ss, setter), ON[takes]) == want, (sorted(has), takes)
            assert ss.options.has(ss.masked) == (has if want is not None else has | {takes})
            assert fake_set.calls == ([] if want is not None else ['nfa_specset_' + setter])
            for off in OFF[takes]:
                getattr(ss, setter)(off)
                assert getattr(ss, takes) is None and ss.options.has(ss.masked) == has - {takes}
    assert 0 < n_refused < 1024 * 8
    assert all(opt.refusal(takes, frozenset()) is None for takes in opt.OPTION_NAMES)
    assert all(opt.refusal('layered', has) is None and opt.refusal('nonsense', has) is None for has in subsets())


def test_an_incompatible_pair_is_refused_in_either_order():
    """As for the engine's table (test_set_rules_cpu.py): 19 pairs, each from both sides; masked channels from one."""
    pairs = [(a, b) for a, b in itertools.permutations(opt.OPTION_NAMES, 2) if opt.refusal(b, {a}) is not None]
    assert len(pairs) == 2 * (7 + 5 + 2 + 4 + 1) and all((b, a) in pairs for a, b in pairs)
    assert opt.refusal('calibration', {'noise_uncertainty'}) == opt.refusal('noise_uncertainty', {'calibration'}) == NUNC_CALIB
    assert [t for t in opt.OPTION_NAMES if opt.refusal(t, {'masked'})] == ['correlation', 'response']
