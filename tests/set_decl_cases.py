"""Declarations of spectra sets for the tests of csrc/nfa_set_decl.h and of the seven creators of include/nestfit_amd.h: a
declaration is a dict of the fields of SetDecl (numpy arrays, numbers, None for a null pointer), `call_creator` hands one to a
loaded engine library, and REFUSALS lists every refusal of the creators with the literal message -- taken from the source of
the creators while they were seven functions that called each other -- plus, for every route and noise kind, one doubly wrong
input per adjacent pair of checks with the message that wins.  No GPU is needed to import this module."""
import ctypes as C

import numpy as np

WHO = ('model', 'channel_noise', 'lines', 'lte', 'bands', 'mix', 'filled')     # SetCreator, csrc/nfa_set_decl.h
ENTRY = {'create': 'nfa_specset_create', 'model': 'nfa_specset_create_model', 'channel_noise': 'nfa_specset_create_channel_noise',
         'lines': 'nfa_specset_create_lines', 'lte': 'nfa_specset_create_lte', 'bands': 'nfa_specset_create_lte_bands',
         'mix': 'nfa_specset_create_lte_mix', 'filled': 'nfa_specset_create_lte_filled'}
INT32 = ('trans_ids', 'n_trans', 'n_lines', 'species', 'n_q')
FLOAT = ('rest_freqs', 'voff', 'tau_wts', 'e_up', 'g_up', 'a_ul', 'q_temp', 'q_val', 'data', 'noise', 'chan_noise')
FIELDS = ('who', 'out', 'model', 'n_spec', 'sizes', 'trans_ids', 'rest_freqs', 'n_trans', 'n_lines', 'voff', 'tau_wts', 'e_up', 'g_up',
          'a_ul', 'n_species', 'species', 'n_q', 'q_temp', 'q_val', 'xarr', 'n_pix', 'data', 'noise', 'chan_noise')
CKMS = 299792.458

Q_TEMP, Q_VAL = (5.0, 10.0, 20.0), (1.0, 2.0, 4.0)
Q2_TEMP, Q2_VAL = (5.0, 10.0), (1.5, 3.0)


def declaration(who, **fields):
    d = dict.fromkeys(FIELDS)
    d.update(who=who, out=True, model=0, n_spec=0, n_species=1, n_pix=0)
    d.update(fields)
    return normalised(d)


def normalised(d):
    """The arrays of a declaration as contiguous arrays of the C types."""
    d = dict(d)
    for k in INT32:
        d[k] = None if d[k] is None else np.ascontiguousarray(d[k], dtype=np.int32)
    for k in FLOAT:
        d[k] = None if d[k] is None else np.ascontiguousarray(d[k], dtype=np.float64)
    d['sizes'] = None if d['sizes'] is None else np.ascontiguousarray(d['sizes'], dtype=np.int64)
    d['xarr'] = None if d['xarr'] is None else [np.ascontiguousarray(x, dtype=np.float64) for x in d['xarr']]
    return d


def tables(who, variant=''):
    """The line tables of the small declarations: two spectra; `bands` and beyond with transitions (2, 1) -- or (1, 1), variant
    'flat' -- and `mix` and `filled` with two species, or one, variant 'one'."""
    t = {}
    if who in ('lines', 'lte'):
        t.update(n_lines=[2, 1], rest_freqs=[1e11, 1.1e11], voff=[0.0, 5.0, 0.0], tau_wts=[0.5, 0.5, 1.0])
        if who == 'lte':
            t.update(e_up=[10.0, 20.0], g_up=[3.0, 5.0], a_ul=[1e-6, 2e-6], n_q=[3], q_temp=Q_TEMP, q_val=Q_VAL)
    elif who in ('bands', 'mix', 'filled'):
        if 'flat' in variant:
            t.update(n_trans=[1, 1], n_lines=[2, 1], rest_freqs=[1e11, 1.1e11], voff=[0.0, 5.0, 0.0], tau_wts=[0.5, 0.5, 1.0],
                     e_up=[10.0, 20.0], g_up=[3.0, 5.0], a_ul=[1e-6, 2e-6])
        else:
            t.update(n_trans=[2, 1], n_lines=[1, 1, 1], rest_freqs=[1.00005e11, 1.00006e11, 1.1e11], voff=[0.0, 0.0, 0.0],
                     tau_wts=[1.0, 1.0, 1.0], e_up=[10.0, 20.0, 30.0], g_up=[3.0, 5.0, 7.0], a_ul=[1e-6, 2e-6, 3e-6])
        t.update(n_q=[3], q_temp=Q_TEMP, q_val=Q_VAL)
        if who != 'bands':
            n = len(t['n_lines'])
            if 'one' in variant:
                t.update(n_species=1, species=[0] * n)
            else:
                t.update(n_species=2, species=[0] * (n - 1) + [1], n_q=[3, 2], q_temp=Q_TEMP + Q2_TEMP, q_val=Q_VAL + Q2_VAL)
    return t


def small(who, chan=False, variant=''):
    """The smallest valid declaration of a creator: two spectra of 2 and 3 channels, one pixel."""
    entry = who
    who = 'model' if who == 'create' else who
    d = dict(n_spec=2, sizes=[2, 3], xarr=[[1e11, 1.0001e11], [1.1e11, 1.1001e11, 1.1002e11]], n_pix=1, data=np.zeros(5),
             noise=None if chan else [0.1, 0.2], chan_noise=np.full(5, 0.1) if chan else None)
    if who in ('model', 'channel_noise'):
        d.update(trans_ids=[1, 2])
    d.update(tables(who, variant))
    d = declaration(who, **d)
    d['entry'] = ENTRY[entry]
    return d


def edited(d, edits):
    """A copy of declaration d with (field, index or None, value) edits; a value that is callable gets the old one."""
    d = {k: (v.copy() if isinstance(v, np.ndarray) else list(v) if isinstance(v, list) else v) for k, v in d.items()}
    for key, idx, val in edits:
        if idx is None:
            d[key] = val(d[key]) if callable(val) else val
        elif key == 'xarr':
            d[key][idx] = val(d[key][idx]) if callable(val) else val
        else:
            d[key][idx] = val
    entry = d.pop('entry')
    d = normalised(d)
    d['entry'] = entry
    return d


# ---------------------------------------------------------------------------- the refusals
NULL = 'null argument'
ONE = 'exactly one of noise and chan_noise must be given'
N_SPEC = 'n_spec must be in 1..16'
N_PIX = 'n_pix must be >= 1'
SIZE = 'spectrum size out of range'
AXIS = 'frequency axis must be ascending'
NOISE = 'noise must be > 0'
CHAN = 'channel noise must be > 0 (NaN is not allowed; inf masks the channel)'
NAN_DATA = 'NaN data in a channel that is not masked (channel noise inf masks it)'
MASKED = 'every channel of a spectrum is masked (channel noise inf)'
M_HYPERFINE = 'the hyperfine model takes its line tables through nfa_specset_create_lines'
M_LTE = 'unknown model to this creator: the LTE model takes its line tables and partition function through nfa_specset_create_lte'
M_UNKNOWN = 'unknown model'
GAUSS = 'the Gaussian model takes one spectrum'
T_NH3, T_N2HP = 'trans_id must be in 1..9', 'trans_id must be in 1..3'
L_COUNT = 'a line table must have 1..50 lines'
L_NU = 'a rest frequency must be finite and positive'
L_VOFF = 'a velocity offset must be finite and below the speed of light'
L_WT = 'a line weight must be finite and not negative'
L_ZERO = 'the weights of a line table are all zero'
T_EUP = 'an upper-level energy must be finite and not negative (K)'
T_GUP = 'an upper-level weight must be finite and positive'
T_AUL = 'an Einstein coefficient must be finite and positive (1/s)'
T_SUM = 'the weights of a transition must sum to 1 within 1e-6'
Q_N = 'a partition table must have 2..64 entries'
Q_T = 'the temperatures of a partition table must be finite, positive and strictly ascending'
Q_V = 'a partition function value must be finite and positive'
B_NT = 'a spectrum must have 1..8 transitions'
B_50 = 'the transitions of a spectrum must have at most 50 lines together'
B_TWICE = 'a spectrum lists the same transition twice'
X_TWICE = 'a spectrum lists the same transition of a species twice'
X_N = 'n_species must be in 1..4'
X_INDEX = 'a species index must be in 0..n_species - 1'
X_NONE = 'a species without a transition in any spectrum: its column density would be unconstrained'

rev = lambda x: x[::-1].copy()       # noqa: E731


def step(message, *edits, pair=True):
    """One check of a route: the edits that fail it on a valid declaration, and whether the same edits still fail it first beside the
    next step's (false where the next check replaces this one, like the Gaussian model's, which needs no trans_ids)."""
    return message, list(edits), pair


def tail(chan):
    """The checks behind the tables, the same for every creator: a scalar noise is checked last, a noise per channel before the axes."""
    if chan:
        return [step(N_PIX, ('n_pix', None, 0)), step(SIZE, ('sizes', 0, 1)), step(SIZE, ('sizes', 1, 1)), step(CHAN, ('chan_noise', 0, 0.0)),
                step(NAN_DATA, ('data', 1, np.nan)), step(MASKED, ('chan_noise', slice(2, 5), np.inf)), step(AXIS, ('xarr', 0, rev)),
                step(AXIS, ('xarr', 1, rev))]
    return [step(N_PIX, ('n_pix', None, 0)), step(SIZE, ('sizes', 0, 1)), step(AXIS, ('xarr', 0, rev)), step(SIZE, ('sizes', 1, 1)),
            step(AXIS, ('xarr', 1, rev)), step(NOISE, ('noise', 0, 0.0))]


def model_steps(chan):
    return [step(M_HYPERFINE, ('model', None, 3)), step(M_LTE, ('model', None, 4)), step(M_UNKNOWN, ('model', None, 7)),
            step(NULL, ('trans_ids', None, None), pair=False), step(GAUSS, ('model', None, 2))]


def table_steps(at):
    """check_one_table on the first table, then on the second (`at`: how a message names tables 0 and 1; table 0 has the lines
    [0, n0))."""
    return lambda n0: [step(L_COUNT + at[0], ('n_lines', 0, 0)), step(L_NU + at[0], ('rest_freqs', 0, -1.0)), step(L_VOFF + at[0], ('voff', 0, np.inf)),
                       step(L_WT + at[0], ('tau_wts', 0, -1.0)), step(L_ZERO + at[0], ('tau_wts', slice(0, n0), 0.0))]


def transition_steps(at):
    """check_one_transition on the first transition"""
    return [step(T_EUP + at, ('e_up', 0, -1.0)), step(T_GUP + at, ('g_up', 0, 0.0)), step(T_AUL + at, ('a_ul', 0, 0.0)),
            step(T_SUM + at, ('tau_wts', 0, 0.6))]


def partition_steps(at=''):
    return [step(Q_N + at, ('n_q', 0, 1)), step(Q_T + at, ('q_temp', 0, -1.0)), step(Q_V + at, ('q_val', 0, 0.0)), step(Q_T + at, ('q_temp', 1, 5.0))]


def prefix(who, chan):
    both = ('noise', None, np.array([0.1, 0.2])) if chan else ('chan_noise', None, np.full(5, 0.1))
    steps = [step(NULL, ('out', None, False))]
    if who in ('mix', 'filled'):
        steps.append(step(X_N, ('n_species', None, 0)))
    steps += [step(ONE, both), step(N_SPEC, ('n_spec', None, 0))]
    if who in ('bands', 'mix', 'filled'):
        steps.append(step(B_NT + ' (spectrum 0)', ('n_trans', 0, 0)))
    return steps


def flat_route(who, chan, variant):
    """Every table, then every transition: the LTE creator's order, which a bands declaration with a transition per spectrum and a
    mix declaration of one species with a transition per spectrum take too."""
    s0, s1 = ' (spectrum 0)', ' (spectrum 1)'
    steps = prefix(who, chan) + table_steps((s0, s1))(2) + [step(L_COUNT + s1, ('n_lines', 1, 0))]
    if who != 'lines':
        steps += [step(NULL, ('e_up', None, None))] + transition_steps(s0) + [step(T_EUP + s1, ('e_up', 1, -1.0))] + partition_steps()
    return steps + tail(chan)


def banded_route(who, chan, variant):
    """Transition by transition: band_layout's order.  `mixed`: the set keeps its mix record (two species, or a filled set), whose
    messages name the species."""
    mixed = who == 'filled' or (who == 'mix' and 'one' not in variant)
    flat = 'flat' in variant
    t0, t1 = ' (spectrum 0, transition 0)', (' (spectrum 1, transition 0)' if flat else ' (spectrum 0, transition 1)')
    steps = prefix(who, chan)
    if who in ('mix', 'filled'):
        steps.append(step(X_INDEX + ' (transition 0)', ('species', 0, -1)))
        if 'one' not in variant:
            steps.append(step(X_NONE + ' (species 1)', ('species', -1, 0)))
    steps += [step(NULL, ('e_up', None, None))] + table_steps((t0, t1))(2 if flat else 1) + transition_steps(t0)
    steps.append(step(L_COUNT + t1, ('n_lines', 1, 0)))
    if not flat:
        steps.append(step((X_TWICE if mixed else B_TWICE) + t1, ('rest_freqs', 1, 1.00005e11), ('e_up', 1, 10.0), ('g_up', 1, 3.0), ('a_ul', 1, 1e-6)))
        steps.append(step(L_COUNT + ' (spectrum 1, transition 0)', ('n_lines', 2, 0)))
    steps += partition_steps(' (species 0)' if mixed else '')
    if mixed and 'one' not in variant:
        steps.append(step(Q_N + ' (species 1)', ('n_q', 1, 1)))
    return steps + tail(chan)


def routes():
    """(name, valid declaration, steps in the frozen order) of every route and noise kind."""
    d = small('create')
    yield 'create', d, ([step(NULL, ('out', None, False)), step(NULL, ('trans_ids', None, None)), step(N_SPEC, ('n_spec', None, 0))]
                        + tail(False)[:2] + [step(T_NH3, ('trans_ids', 0, 0))] + tail(False)[2:4] + [step(T_NH3, ('trans_ids', 1, 10))] + tail(False)[4:])
    t = tail(False)
    yield 'model', small('model'), ([step(NULL, ('out', None, False))] + model_steps(False) + [step(N_SPEC, ('n_spec', None, 0))] + t[:2]
                                    + [step(T_NH3, ('trans_ids', 0, 0))] + t[2:4] + [step(T_NH3, ('trans_ids', 1, 10))] + t[4:])
    t = tail(True)
    yield 'channel_noise', small('channel_noise', True), ([step(NULL, ('out', None, False)), step(N_SPEC, ('n_spec', None, 0))] + t[:6] + model_steps(True)
                                                          + [step(T_NH3, ('trans_ids', 0, 0)), t[6], step(T_NH3, ('trans_ids', 1, 10)), t[7]])
    for chan in (False, True):
        kind = 'channel' if chan else 'scalar'
        yield f'lines/{kind}', small('lines', chan), flat_route('lines', chan, '')
        yield f'lte/{kind}', small('lte', chan), flat_route('lte', chan, '')
        yield f'bands/{kind}', small('bands', chan), banded_route('bands', chan, '')
        yield f'bands flat/{kind}', small('bands', chan, 'flat'), flat_route('bands', chan, 'flat')
        yield f'mix/{kind}', small('mix', chan), banded_route('mix', chan, '')
        yield f'mix one/{kind}', small('mix', chan, 'one'), banded_route('mix', chan, 'one')
        yield f'mix one flat/{kind}', small('mix', chan, 'one flat'), flat_route('mix', chan, 'one flat')
        yield f'filled/{kind}', small('filled', chan), banded_route('filled', chan, '')
        yield f'filled one flat/{kind}', small('filled', chan, 'one flat'), banded_route('filled', chan, 'one flat')


def _clash(a, b):
    """Two steps edit the same thing."""
    return any(ka == kb and (ia is None or ib is None or ia == ib or isinstance(ia, slice) or isinstance(ib, slice)) for ka, ia, _ in a for kb, ib, _ in b)


def singles():
    """Refusals outside the walk along the routes: the other values of a check, and every pointer of the null lists."""
    m, c = small('model'), small('channel_noise', True)
    yield 'model n_spec 17', edited(m, [('n_spec', None, 17)]), N_SPEC
    yield 'model -1', edited(m, [('model', None, -1)]), M_UNKNOWN
    yield 'model N2H+ trans_id', edited(m, [('model', None, 1), ('trans_ids', 0, 4)]), T_N2HP
    yield 'model NaN noise', edited(m, [('noise', 1, np.nan)]), NOISE
    yield 'model size above 2^24', edited(m, [('sizes', 1, (1 << 24) + 1)]), SIZE
    yield 'model equal channels', edited(m, [('xarr', 0, np.array([1e11, 1e11]))]), AXIS
    yield 'channel NaN noise', edited(c, [('chan_noise', 3, np.nan)]), CHAN
    yield 'channel negative noise', edited(c, [('chan_noise', 4, -1.0)]), CHAN
    for who in ('model', 'channel_noise', 'lines', 'lte', 'bands', 'mix', 'filled'):
        for chan in ((True,) if who == 'channel_noise' else (False,) if who == 'model' else (False, True)):
            d = small(who, chan)
            nulls = ['sizes', 'xarr', 'data'] + (['noise'] if who == 'model' else ['chan_noise'] if who == 'channel_noise' else
                                                 ['n_lines', 'rest_freqs', 'voff', 'tau_wts'])
            nulls += ['n_trans'] if who in ('bands', 'mix', 'filled') else []
            nulls += ['species', 'n_q'] if who in ('mix', 'filled') else []
            for k in nulls:
                yield f'{who} null {k}', edited(d, [(k, None, None)]), NULL
            if who in ('lte', 'bands', 'mix', 'filled'):
                for k in ('g_up', 'a_ul', 'q_temp', 'q_val'):
                    yield f'{who} null {k}', edited(d, [(k, None, None)]), NULL
    lte = small('lte')
    yield 'lte n_q 65', edited(lte, [('n_q', 0, 65)]), Q_N
    yield 'lte equal logarithms', edited(lte, [('q_temp', None, np.array([1e300, np.nextafter(1e300, np.inf), 2e300]))]), Q_T
    yield 'lte lines 51', edited(lte, [('n_lines', 0, 51)]), L_COUNT + ' (spectrum 0)'
    yield 'lte offset at c', edited(lte, [('voff', 1, CKMS)]), L_VOFF + ' (spectrum 0)'
    yield 'lte weight of the second line', edited(lte, [('tau_wts', 1, np.nan)]), L_WT + ' (spectrum 0)'
    bands = small('bands')
    yield 'bands 9 transitions', edited(bands, [('n_trans', 1, 9)]), B_NT + ' (spectrum 1)'
    many = dict(n_lines=np.array([30, 30, 1]), voff=np.zeros(61), tau_wts=np.concatenate([np.full(30, 1 / 30), np.full(30, 1 / 30), [1.0]]))
    yield 'bands 60 lines', edited(bands, [(k, None, v) for k, v in many.items()]), B_50 + ' (spectrum 0)'
    mix = small('mix')
    yield 'mix n_species 5', edited(mix, [('n_species', None, 5)]), X_N
    yield 'mix species 2', edited(mix, [('species', 1, 2)]), X_INDEX + ' (transition 1)'
    yield 'mix species 0 unseen', edited(mix, [('species', None, np.array([1, 1, 1]))]), X_NONE + ' (species 0)'
    yield 'mix second table', edited(mix, [('q_val', 4, -1.0)]), Q_V + ' (species 1)'
    # the same numbers in two species are two transitions
    yield 'mix twice across species', edited(mix, [('n_trans', None, np.array([1, 2])), ('rest_freqs', 2, 1.00006e11), ('e_up', 2, 20.0),
                                                   ('g_up', 2, 5.0), ('a_ul', 2, 2e-6), ('n_pix', None, 0)]), N_PIX


def refusals():
    """[(label, declaration, NFA_ERR_ARG, message)]: every step of every route alone, and beside the step after it."""
    out = []
    for name, valid, steps in routes():
        for k, (message, edits, pair) in enumerate(steps):
            out.append((f'{name}: {message}', edited(valid, edits), 1, message))
            if pair and k + 1 < len(steps) and not _clash(edits, steps[k + 1][1]):
                out.append((f'{name}: {message} + {steps[k + 1][0]}', edited(valid, edits + steps[k + 1][1]), 1, message))
    out += [(label, d, 1, message) for label, d, message in singles()]
    return out


REFUSALS = refusals()
VALID = [(name, valid) for name, valid, _ in routes()]


# ---------------------------------------------------------------------------- the engine's creators
def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def call_creator(lib, d, handle=None):
    """The creator d['entry'] of a loaded engine library with declaration d: (rc, message, handle); the set is the caller's."""
    h = C.c_void_p() if handle is None else handle
    out = C.byref(h) if d['out'] else None
    xp = None if d['xarr'] is None else (C.POINTER(C.c_double) * len(d['xarr']))(*[_ptr(x, C.c_double) for x in d['xarr']])
    dp, ip = (lambda k: _ptr(d[k], C.c_double)), (lambda k: _ptr(d[k], C.c_int32))
    head = (out, d['n_spec'], _ptr(d['sizes'], C.c_int64))
    base = (xp, d['n_pix'], dp('data'))
    both = (dp('noise'), dp('chan_noise'))
    lte = (dp('e_up'), dp('g_up'), dp('a_ul'))
    lines = (ip('n_lines'), dp('rest_freqs'), dp('voff'), dp('tau_wts'))
    entry = d['entry']
    fn = getattr(lib, entry)
    if entry == 'nfa_specset_create':
        rc = fn(*head, ip('trans_ids'), *base, dp('noise'))
    elif entry == 'nfa_specset_create_model':
        rc = fn(out, d['model'], *head[1:], ip('trans_ids'), dp('rest_freqs'), *base, dp('noise'))
    elif entry == 'nfa_specset_create_channel_noise':
        rc = fn(out, d['model'], *head[1:], ip('trans_ids'), dp('rest_freqs'), *base, dp('chan_noise'))
    elif entry == 'nfa_specset_create_lines':
        rc = fn(*head, *lines, *base, *both)
    elif entry == 'nfa_specset_create_lte':
        rc = fn(*head, *lines, *lte, 0 if d['n_q'] is None else int(d['n_q'][0]), dp('q_temp'), dp('q_val'), *base, *both)
    elif entry == 'nfa_specset_create_lte_bands':
        rc = fn(*head, ip('n_trans'), *lines, *lte, 0 if d['n_q'] is None else int(d['n_q'][0]), dp('q_temp'), dp('q_val'), *base, *both)
    else:
        rc = fn(*head, ip('n_trans'), *lines, *lte, d['n_species'], ip('species'), ip('n_q'), dp('q_temp'), dp('q_val'), *base, *both)
    return rc, lib.nfa_last_error().decode(), h


# ---------------------------------------------------------------------------- sets that run: the shapes of tests/test_set_creation.py
NAMES = ('ammonia', 'n2hp', 'gaussian', 'lines', 'lte', 'bands', 'mix', 'filled')
N_ROWS = 16
# a component's parameters, the first and the second component (parameter-major rows: include/nestfit_amd.h)
VOFF, SIGM, TEX = (0.5, -0.8), (0.4, 0.6), (6.0, 7.5)
PARS = {'ammonia': [VOFF, (12.0, 15.0), TEX, (14.5, 14.2), SIGM, (0.5, 0.3)], 'n2hp': [VOFF, TEX, (0.3, 0.0), SIGM],
        'gaussian': [VOFF, (0.8, 0.5), (2.0, 1.0)], 'lines': [VOFF, TEX, (0.3, 0.0), SIGM], 'lte': [VOFF, TEX, (13.5, 13.2), SIGM]}
PARS['bands'] = PARS['lte']
PARS['mix'] = PARS['lte'] + [(13.3, 13.0)]
PARS['filled'] = PARS['mix'] + [(-0.3, -0.1)]


def axis(nu, n):
    """n channels of 0.3 km/s about the rest frequency nu"""
    return nu * (1.0 + (np.arange(n) - n // 2) * (0.3 / CKMS))


def builtin_nu(lib, model, trans_id):
    nu, n, buf = C.c_double(), C.c_int(), np.zeros((2, 50))
    assert lib.nfa_builtin_lines(model, trans_id, C.byref(nu), _ptr(buf[0], C.c_double), _ptr(buf[1], C.c_double), C.byref(n)) == 0
    return nu.value


def full(name, lib):
    """A valid declaration with a scalar noise of creator `name`: two pixels of two spectra of 64 and 130 channels (130 crosses a
    row of 64; the Gaussian model's one spectrum has 130), up to three transitions in a spectrum, two species."""
    rng = np.random.default_rng(NAMES.index(name) + 11)
    sizes = [130] if name == 'gaussian' else [64, 130]
    n_spec, tot = len(sizes), sum(sizes)
    d = dict(n_spec=n_spec, sizes=sizes, n_pix=2, data=rng.normal(0.0, 0.1, (2, tot)), noise=[[0.1, 0.2], [0.15, 0.12]] if n_spec == 2 else [[0.1], [0.15]])
    if name in ('ammonia', 'n2hp'):
        model = NAMES.index(name)
        d.update(model=model, trans_ids=[1, 2], xarr=[axis(builtin_nu(lib, model, t), n) for t, n in zip((1, 2), sizes)])
        return dict(declaration('model', **d), entry=ENTRY['create' if name == 'ammonia' else 'model'])
    if name == 'gaussian':
        d.update(model=2, rest_freqs=[1e11], xarr=[axis(1e11, 130)])
        return dict(declaration('model', **d), entry=ENTRY['model'])
    nus = [1e11, 1.1e11]
    d.update(xarr=[axis(nu, n) for nu, n in zip(nus, sizes)])
    if name in ('lines', 'lte'):
        d.update(n_lines=[3, 2], rest_freqs=nus, voff=[0.0, 2.5, -3.0, 0.0, 4.0], tau_wts=[0.5, 0.3, 0.2, 0.6, 0.4])
        if name == 'lte':
            d.update(e_up=[10.0, 20.0], g_up=[3.0, 5.0], a_ul=[1e-5, 2e-5], n_q=[3], q_temp=Q_TEMP, q_val=Q_VAL)
    else:       # three transitions in the first spectrum (the caller's order is not the engine's), two in the second
        d.update(n_trans=[3, 2], n_lines=[1, 2, 1, 2, 1], rest_freqs=[1e11 + 1.0e6, 1e11 - 1.5e6, 1e11, 1.1e11, 1.1e11 + 2.0e6],
                 voff=[0.0, 1.0, -1.0, 0.0, 0.0, 2.0, 0.0], tau_wts=[1.0, 0.25, 0.75, 1.0, 0.5, 0.5, 1.0],
                 e_up=[30.0, 10.0, 20.0, 15.0, 25.0], g_up=[7.0, 3.0, 5.0, 4.0, 6.0], a_ul=[3e-5, 1e-5, 2e-5, 1.5e-5, 2.5e-5], n_q=[3], q_temp=Q_TEMP, q_val=Q_VAL)
        if name != 'bands':
            d.update(n_species=2, species=[1, 0, 0, 0, 1], n_q=[3, 2], q_temp=Q_TEMP + Q2_TEMP, q_val=Q_VAL + Q2_VAL)
    return dict(declaration(name, **d), entry=ENTRY[name])


def per_channel(d, masked=False):
    """Declaration d with its noise per channel: the same constant in every channel of a (pixel, spectrum) -- or, `masked`, a noise
    that varies along the spectra with a masked channel in the second spectrum of pixel 1, whose data are NaN."""
    noise = np.repeat(d['noise'].reshape(d['n_pix'], d['n_spec']), d['sizes'], axis=1)
    data = d['data']
    if masked:
        noise = noise * (1.0 + 0.5 * np.sin(np.arange(noise.shape[1]) / 5.0) ** 2)
        noise[1, -3] = np.inf
        data = data.reshape(noise.shape).copy()
        data[1, -3] = np.nan
    e = dict(d, noise=None, chan_noise=np.ascontiguousarray(noise), data=data)
    if d['who'] == 'model':
        e.update(who='channel_noise', entry=ENTRY['channel_noise'])
    return e


def thetas(name, ncomp):
    """N_ROWS parameter rows about PARS[name], parameter-major"""
    rng = np.random.default_rng(100 * NAMES.index(name) + ncomp)
    base = np.array([p[c] for p in PARS[name] for c in range(ncomp)])
    return np.ascontiguousarray(base + 0.02 * rng.normal(size=(N_ROWS, base.size)))


def evaluate(lib, d, name, ncomp):
    """The set of declaration d made, run and destroyed: (spectra and lnL of predict_batch for thetas(name, ncomp) against
    pixels 0, 1, 0, ..., null_lnZ), as bytes."""
    rc, msg, h = call_creator(lib, d)
    assert rc == 0, msg
    run = C.c_void_p()
    try:
        assert lib.nfa_runner_create(C.byref(run), h, None, ncomp, 0, 0) == 0, lib.nfa_last_error().decode()
        th = thetas(name, ncomp)
        pix = np.ascontiguousarray(np.arange(N_ROWS) % 2, dtype=np.int32)
        spec, lnl, null = np.empty((N_ROWS, int(d['sizes'].sum()))), np.empty(N_ROWS), np.empty((d['n_pix'], d['n_spec']))
        assert lib.nfa_runner_predict_batch(run, _ptr(pix, C.c_int32), _ptr(th, C.c_double), N_ROWS, _ptr(spec, C.c_double), _ptr(lnl, C.c_double)) == 0, \
            lib.nfa_last_error().decode()
        assert lib.nfa_runner_synchronize(run) == 0
        assert lib.nfa_specset_null_lnz(h, _ptr(null, C.c_double)) == 0
        return spec, lnl, null
    finally:
        if run:
            lib.nfa_runner_destroy(run)
        lib.nfa_specset_destroy(h)
